"""CPU check of the planner's ragged-width chain rule (tpp-mlir_amd/csrc/gemm_plan.cpp chain_ragged_b_kind / plan_chain_ragged,
xsmm_hip_set_chain_ragged): tests/gemm_plan_chain_ragged/driver.cpp, compiled with the library's flags, steps layer chains - m around every BM, n in
{BN, BN + 8, BN + 4, 2 BN + 24, 1000} and the k classes with each tile forced, the GPU test's other chains with the three B images, the rows
of the A/B, the chains the other rules keep, and one refusal each - through both functions, and through plan_chain_edge and
plan_chain_rounds on the same chains, at 256, 64 and 304 compute units. One line per chain and CU count;
tests/golden/gemm_plan_chain_ragged.txt is the reviewed record. Whatever the table says, every line must also satisfy the rule as restated here
from its issue; every refusal is reached; with the switch off - and on - the answers of plan_chain_edge and plan_chain_rounds are those of
tests/golden/gemm_plan_chain_edge.txt and _rounds.txt wherever lines coincide; and tests/golden/gemm_plan.txt is what it was.
And, compile-only: the translation unit of the mode holds exactly the instances its table names, none with scratch."""
import difflib
import hashlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_chain_ragged.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402
import blw_codeobj  # noqa: E402

LINE = re.compile(r'^(\d+)x(\d+) k([\d,]+) br([\d,]+) (f32|bf16) vf(\d) f(-?\d+) sw([01]) ce([01]) cr(\d+) et(-?\d) st([01]) x(\d+) cus(\d+) : v(\d+),(-?\d+) gf([01]) kind(-?\d) "([^"]*)" \| '
                  r'tile(-?\d) "([^"]*)"(?: \| edge kind(-?\d) "([^"]*)" tile(-?\d) "([^"]*)" \| rounds pt(-?\d) tile(-?\d) G(\d+) R(\d+) g([01]) "([^"]*)")?$')
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]
WHYS_PLAN = ["ragged-width chains are off", "strict mode", "fewer than 2 or more than 8 calls", "k below 64 or not a multiple of 8, or an empty batch", "n is not a multiple of 8",
             "do not share one B image", "m or n is below every tile", "more tiles than compute units", "not a ragged-width chain", "gate: "]
WHYS_KIND = ["ragged-width chains are off", "an f32 call", "stores a VNNI C or is not beta 0", "a forced kernel", "k below 64 or not a multiple of 8", "off the grid"]


def exists(t, kind):
    """the instances of the mode: tiles 0 .. 3 x the three images, less 64x128 with VNNI-2 (it would need scratch)"""
    return 0 <= t <= 3 and kind in (0, 2, 4) and not (t == 2 and kind == 0)


def chain_ragged_rule(m, n, ks, brs, cus, kind, forced_tile=None, strict=False, sw=1):
    """the tile a ragged-width chain takes, None = call by call - restated from the issue. A tile fits when its instance exists, m >= BM,
    n >= BN and ceil(m / BM) * ceil(n / BN) <= CUs; the forced tile if it fits, else the smallest that fits - gated where that is 128x128
    only because 64x128 has no instance for the image; never with the switch off, in
    strict mode, with fewer than 2 or more than 8 calls, a k below 64 or no multiple of 8, an empty batch or n % 8 != 0; and a chain with
    n % BN == 0 and every k % 64 == 0 is another rule's business"""
    if not sw or strict or not 2 <= len(ks) <= 8 or any(k < 64 or k % 8 for k in ks) or any(b < 1 for b in brs) or n % 8:
        return None
    fits = [t for t, (bm, bn) in enumerate(TILE) if exists(t, kind) and m >= bm and n >= bn and -(-m // bm) * -(-n // bn) <= cus]
    if not fits:
        return None
    t = forced_tile if forced_tile in fits else fits[0]
    if forced_tile is None:  # the gates (a forcing edge-tile mode is not gated, whichever tile fits)
        bm2, bn2 = TILE[2]
        if t == 3 and not exists(2, kind) and m >= bm2 and n >= bn2 and -(-m // bm2) * -(-n // bn2) <= cus:
            return None  # the gate: 64x128 by the rule, no such instance for the image, 128x128 measured slower than call by call
        if t in (0, 1) and any(k % 64 == 0 and (b * (k // 64)) % 2 == 0 for k, b in zip(ks, brs)):
            return None  # the second gate: a whole-k layer that runs two chunks per barrier as a single call (tiles 32x64, 64x64)
    return t if n % TILE[t][1] or any(k % 64 for k in ks) else None


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_chain_ragged")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_chain_ragged", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_chain_ragged")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    out = []
    names = ("m n ks brs dt vf forced sw ce cr et strict extra cus v0 v1 gf kind kind_why tile tile_why ekind ekind_why etile etile_why pt rtile G R gated rwhy").split()
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "unreadable line: " + l
        r = dict(zip(names, m.groups()))
        for k in r:
            if k in ("ks", "brs"):
                r[k] = [int(x) for x in r[k].split(",")]
            elif k not in ("dt", "kind_why", "tile_why", "ekind_why", "etile_why", "rwhy") and r[k] is not None:
                r[k] = int(r[k])
        r["line"] = l
        out.append(r)
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's ragged-width choices differ from tests/golden/gemm_plan_chain_ragged.txt:\n" + diff)


def test_every_line_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        image = {2: 0, 0: 2, 4: 4}[r["vf"]]
        differ = "differ" in r["kind_why"]
        want = None if differ else chain_ragged_rule(r["m"], r["n"], r["ks"], r["brs"], r["cus"], image, r["et"] if r["et"] >= 0 else None, bool(r["strict"]), r["sw"])
        assert r["tile"] == (-1 if want is None else want), (want, r["line"])
        assert (r["tile"] >= 0) == (r["tile_why"] == ""), r["line"]
        if r["tile"] >= 0:
            chosen += 1
            bm, bn = TILE[r["tile"]]
            assert exists(r["tile"], image) and r["m"] >= bm and r["n"] >= bn and -(-r["m"] // bm) * -(-r["n"] // bn) <= r["cus"], r["line"]
            assert r["n"] % bn or any(k % 64 for k in r["ks"]), r["line"]
        # a call's B image: none with the switch off, for f32, beta 1, a VNNI C, a forced kernel, a k below 64 or off 8, an operand off the grid
        forced_kernel = r["forced"] == 8 or (r["forced"] >= 0 and r["v0"] == r["forced"])
        if r["kind"] >= 0:
            assert r["sw"] and r["dt"] == "bf16" and not forced_kernel and all(k >= 64 and k % 8 == 0 for k in r["ks"]) and r["n"] % 8 == 0 and r["kind"] == image, r["line"]
        assert (r["kind"] >= 0) == (r["kind_why"] == ""), r["line"]
    assert chosen > 50


def test_every_refusal_is_reached_and_the_case_list_covers_what_the_issue_names(rows):
    for w in WHYS_PLAN:
        assert any(w in r["tile_why"] for r in rows), w
    for w in WHYS_KIND + ["differ in kind"]:
        assert any(w in r["kind_why"] for r in rows), w
    assert {r["tile_why"] for r in rows if r["tile"] < 0} == {r["tile_why"] for r in rows if r["tile"] < 0 and any(w in r["tile_why"] for w in WHYS_PLAN)}, "a why the test does not know"
    assert {r["cus"] for r in rows} == {64, 256, 304}
    for t, (bm, bn) in enumerate(TILE):
        ms = {r["m"]: r["tile"] for r in rows if (r["n"], r["et"], r["ks"][0]) == (bn + 8, t, 72)}  # m around BM (VNNI-2: 64x128 forced falls to 32x64)
        own = 0 if t == 2 else t
        assert ms == {bm - 8: (-1 if bm - 8 < 32 else 0), bm: own, bm + 8: own, 3 * bm - 3: own}, (t, ms)
        ns = {r["n"]: r["tile"] for r in rows if (r["m"], r["et"], r["ks"][0]) == (bm + 8, t, 80)}
        assert ns == {bn: own, bn + 4: -1, 2 * bn + 24: own, 1000: own}, (t, ns)
        whole = {r["n"]: r["tile"] for r in rows if (r["m"], r["et"], r["ks"][0]) == (bm + 8, t, 128) and len(r["ks"]) == 3}
        assert whole == {bn + 8: own, bn: -1}, (t, whole)  # (n = BN with every k whole: nothing ragged in width)
    assert {(r["vf"], r["tile"]) for r in rows if r["brs"] == [2, 2, 2]} == {(2, 1), (0, 1), (4, 1)} and any(r["brs"] == [3, 1, 1] and r["tile"] == 1 for r in rows)
    assert any(len(r["ks"]) == 4 and r["tile"] == 1 for r in rows) and any(r["n"] == 192 and r["tile"] == 3 for r in rows)
    assert any(r["sw"] == 0 for r in rows) and any(r["strict"] for r in rows) and any(r["forced"] == 8 for r in rows)
    assert any(r["ce"] == 0 and r["cr"] == 0 for r in rows) and any(r["ce"] == 1 and r["cr"] == 1 for r in rows)

    def pick(m, n, cus=256, et=-1, k0=None, vf=2):
        got = [r for r in rows if (r["m"], r["n"], r["cus"], r["et"], r["vf"]) == (m, n, cus, et, vf) and r["ks"] == [k0 or n, n, n] and r["brs"] == [1, 1, 1] and
               r["sw"] == 1 and r["ce"] == 1 and r["cr"] == 1 and not r["strict"] and r["forced"] == -1 and r["dt"] == "bf16" and r["kind"] >= 0]
        assert got and len({g["tile"] for g in got}) == 1, (m, n, cus, et, len(got))
        return got[0]
    # the 1000-wide MLP: 16 x 16 tiles of 64x64 fill 256 CUs at 1000 and 1024 rows; 2000 rows: 64x128 has no VNNI-2 instance, 16 x 8 of 128x128
    assert [pick(m, 1000)["tile"] for m in (1000, 1024, 2000)] == [1, 1, -1] and pick(2000, 1000)["tile_why"].startswith("gate: "), "2000 rows: gated (measured slower on 128x128)"
    assert pick(2000, 1000, et=3)["tile"] == 3, "a forced tile is not gated"
    assert pick(2000, 1000, vf=0)["tile"] == 2 and pick(2000, 1000, vf=4)["tile"] == 2
    assert pick(4096, 1000)["tile"] == 3 and pick(4100, 1000)["tile"] == -1, "33 x 8 tiles: call by call, never several rounds"
    gated = [r for r in rows if (r["m"], r["n"], r["cus"], r["et"]) == (1024, 1000, 256, -1) and r["ks"] == [64, 1000, 1000] and r["brs"] == [16, 1, 1]]
    assert gated and all(r["tile"] == -1 and "two chunks per barrier" in r["tile_why"] for r in gated), "1024 rows x [1024, 1000, 1000]: gated (measured slower)"
    assert pick(1024, 1000, k0=784)["tile"] == 1 and pick(200, 200)["tile"] == 0 and pick(200, 200, k0=784)["tile"] == 0
    assert pick(1000, 1000, cus=64)["tile"] == 3 and pick(2000, 1000, cus=64)["tile"] == -1
    assert pick(1000, 1000, et=3)["tile"] == 3 and pick(1000, 1000, et=0)["tile"] == 1, "a forced tile that fits; one that does not: the smallest that fits"
    # a chain ragged in m alone and a divisible chain are not this rule's
    assert pick(1000, 1024)["tile"] == -1 and pick(1000, 1024)["etile"] == 1 and pick(1024, 1024)["tile"] == -1 and pick(1024, 1024)["etile"] == -1
    assert pick(4224, 1024)["tile"] == -1 and pick(4224, 1024)["rtile"] == 3 and pick(4224, 1024)["G"] == 17


def _golden_lines(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return {l.split(" : ")[0]: l.rstrip("\n") for l in f if " : " in l}


def test_the_other_chain_rules_answer_as_their_golden_tables_say(rows):
    """the lines of this table that coincide with a line of tests/golden/gemm_plan_chain_edge.txt / _rounds.txt - the same chain, switches, tile
    and CU count -, whatever the new switch: plan_chain_edge's and plan_chain_rounds' answers are the ones recorded there"""
    edge, rounds = _golden_lines("gemm_plan_chain_edge.txt"), _golden_lines("gemm_plan_chain_rounds.txt")
    hits = {(0, "edge"): 0, (1, "edge"): 0, (0, "rounds"): 0, (1, "rounds"): 0}
    for r in rows:
        shape = "%dx%d k%s br%s %s vf%d" % (r["m"], r["n"], ",".join(map(str, r["ks"])), ",".join(map(str, r["brs"])), r["dt"], r["vf"])
        if r["extra"] or r["ekind"] is None:  # (not of the comparison group; beta 1, a VNNI C, an operand off the grid, mixed images: what the other tables' lines do not say)
            continue
        key = "%s f%d sw%d et%d st%d cus%d" % (shape, r["forced"], r["ce"], r["et"], r["strict"], r["cus"])
        if key in edge:
            mine = '%s : v%d gf%d kind%d "%s" | tile%d "%s"' % (key, r["v0"], r["gf"], r["ekind"], r["ekind_why"], r["etile"], r["etile_why"])
            assert mine == edge[key], (mine, edge[key])
            hits[(r["sw"], "edge")] += 1
        key = "%s f%d,%d sw%d st%d cus%d" % (shape, r["forced"], r["forced"], r["cr"], r["strict"], r["cus"])
        if key in rounds:
            mine = '%s : v%d,%d pt%d | tile%d G%d R%d g%d "%s"' % (key, r["v0"], r["v1"], r["pt"], r["rtile"], r["G"], r["R"], r["gated"], r["rwhy"])
            assert mine == rounds[key], (mine, rounds[key])
            hits[(r["sw"], "rounds")] += 1
    assert all(v >= 4 for v in hits.values()), hits


def test_the_single_call_table_is_what_it_was():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan.txt"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == "47d83170a9e065ad7cac7e1f262fe123749fee1f26741562852271ccc04fc960"


_ragged_report = None


def ragged_report():
    """{kernel symbol: (scratch, VGPRs, AGPRs)} of brgemm_bf16_lw_chain_ragged.hip: one device-only compile, shared by the tests of this file"""
    global _ragged_report
    if _ragged_report is None:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(CSRC, "brgemm_bf16_lw_chain_ragged.hip"),
                                "-o", os.path.join(tmp, "k.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        _ragged_report = blw_codeobj._parse(r.stderr)
    return _ragged_report


def test_the_translation_unit_holds_exactly_the_instances_of_its_table_and_no_scratch():
    """brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, 1, true, FLATB, 8>: the four tiles with the loader waves and ring of the divisible
    chain of each, one chunk per barrier, the three B images, less the one instance the table leaves out - no scratch, no AGPRs"""
    rep = ragged_report()
    tiles = sorted({(tile,) + cfg for mode, multi, tile, b_kind, sup, cfg, dims, sym in blw_codeobj.launch_table()[0] if (mode, multi, sup) == (0, 1, 1)})
    assert [t[0] for t in tiles] == [0, 1, 2, 3], tiles
    want = ["_ZN3tpp14brgemm_bf16_lwI" + "".join("Li%dE" % a for a in t[1:]) + "Li1ELb1ELi%dELi8EEEvNS_9ChainArgsE" % image
            for t in tiles for image in (0, 2, 4) if exists(t[0], image)]
    assert len(want) == 11 and sorted(rep) == sorted(want), (sorted(set(rep) - set(want)), sorted(set(want) - set(rep)))
    assert not {n: x for n, x in rep.items() if x[0] or x[1] > 256 or x[2]}, rep
