"""CPU check of the planner's mixed-width chain rule (tpp-mlir_amd/csrc/gemm_plan.cpp plan_chain_widths, xsmm_hip_set_chain_widths):
tests/gemm_plan_chain_widths/driver.cpp, compiled with the library's flags, steps layer chains - the rows of the A/B at 256, 64 and 304 compute
units, the GPU test's chains with every tile forced and the three B images, equal-width chains, and one refusal each - through the rule the
way try_chain_launch asks it. One line per chain and CU count; tests/golden/gemm_plan_chain_widths.txt is the reviewed record. Whatever the
table says, every line must also satisfy the rule as restated here from its issue; every refusal is reached; plan_chain_edge,
plan_chain_rounds and plan_chain_ragged answer on the equal-width chains as tests/golden/gemm_plan_chain_edge.txt, _rounds.txt and
_ragged.txt say wherever lines coincide; and tests/golden/gemm_plan.txt is what it was.
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_chain_widths.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402
import blw_codeobj  # noqa: E402

LINE = re.compile(r'^(\d+) n([\d,]+) k([\d,]+) br([\d,]+) (f32|bf16) vf(\d) f(-?\d+) sw([01]) st([01]) x(\d+) cus(\d+) : v(\d+),(-?\d+) pt(-?\d) kind(-?\d) \| tile(-?\d) "([^"]*)"'
                  r'(?: \| edge tile(-?\d) "([^"]*)" \| rounds tile(-?\d) G(\d+) g([01]) "([^"]*)" \| ragged tile(-?\d) "([^"]*)")?$')
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]
WHYS = ["mixed-width chains are off", "an f32 call", "fewer than 2 or more than 8 calls", "do not share one B image", "k not in 64-k chunks, or an empty batch",
        "every call has the same n", "strict mode", "more tiles than compute units", "no tile divides m and every n", "gate: "]


def widths_rule(m, ns, ks, brs, cus, kind, pt, strict=False, sw=1):
    """the tile a mixed-width chain takes, None = call by call - restated from the issue. 2 .. 8 bf16 calls with one B image, every k >= 64
    and a multiple of 64, every batch >= 1, at least two n differ. A tile fits when BM divides m, BN divides every n and m / BM * max(n) / BN
    <= CUs. The tile all calls were dispatched on if it fits; otherwise never in strict mode, else the smallest tile that fits - gated
    (measured) where some layer alone fits a smaller tile than that."""
    if not sw or pt < -1 or not 2 <= len(ns) <= 8 or kind not in (0, 2, 4) or any(k < 64 or k % 64 for k in ks) or any(b < 1 for b in brs) or len(set(ns)) == 1:
        return None
    fit = lambda t, widths: m % TILE[t][0] == 0 and all(n % TILE[t][1] == 0 for n in widths) and (m // TILE[t][0]) * (max(widths) // TILE[t][1]) <= cus
    fits = [t for t in range(4) if fit(t, ns)]
    if pt in fits:
        return pt
    if strict or not fits:
        return None
    if any(fit(s, [n]) for n in ns for s in range(fits[0])):
        return None  # the gate
    return fits[0]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_chain_widths")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_chain_widths", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_chain_widths")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    out = []
    names = "m ns ks brs dt vf forced sw strict extra cus v0 v1 pt kind tile why etile ewhy rtile G gated rwhy gtile gwhy".split()
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "unreadable line: " + l
        r = dict(zip(names, m.groups()))
        for k in r:
            if k in ("ns", "ks", "brs"):
                r[k] = [int(x) for x in r[k].split(",")]
            elif k not in ("dt", "why", "ewhy", "rwhy", "gwhy") and r[k] is not None:
                r[k] = int(r[k])
        r["line"] = l
        out.append(r)
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's mixed-width choices differ from tests/golden/gemm_plan_chain_widths.txt:\n" + diff)


def test_every_line_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        want = widths_rule(r["m"], r["ns"], r["ks"], r["brs"], r["cus"], r["kind"], r["pt"], bool(r["strict"]), r["sw"])
        assert r["tile"] == (-1 if want is None else want), (want, r["line"])
        assert (r["tile"] >= 0) == (r["why"] == ""), r["line"]
        if r["tile"] >= 0:
            chosen += 1
            bm, bn = TILE[r["tile"]]
            assert r["m"] % bm == 0 and all(n % bn == 0 for n in r["ns"]) and (r["m"] // bm) * (max(r["ns"]) // bn) <= r["cus"], r["line"]
            assert r["dt"] == "bf16" and not r["extra"] and len(set(r["ns"])) > 1, r["line"]
        if r["kind"] >= 0:  # what try_chain_launch hands the rule: one B image of the loader-wave tiles on every call
            assert r["dt"] == "bf16" and not r["extra"] and r["forced"] != 8 and r["kind"] == {2: 0, 0: 2, 4: 4}[r["vf"]], r["line"]
    assert chosen > 100


def test_every_refusal_is_reached_and_the_case_list_covers_what_the_issue_names(rows):
    for w in WHYS:
        assert any(w in r["why"] for r in rows), w
    assert all(any(w in r["why"] for w in WHYS) for r in rows if r["tile"] < 0), "a why the test does not know"
    assert {r["cus"] for r in rows} == {64, 256, 304}

    def pick(m, layers, cus=256, vf=2, forced=-1, sw=1, strict=0):
        got = [r for r in rows if (r["m"], r["ns"], r["ks"], r["cus"], r["vf"], r["forced"], r["sw"], r["strict"]) == (m, layers[1:], layers[:-1], cus, vf, forced, sw, strict) and
               all(b == 1 for b in r["brs"]) and r["dt"] == "bf16" and not r["extra"]]
        assert got and len({g["tile"] for g in got}) == 1, (m, layers, cus, len(got))
        return got[0]
    # the A/B's rows on 256 CUs: the funnel is taken on the smallest tile, the four rows that measured slower are gated
    assert pick(1024, [1024, 512, 256, 128])["tile"] == 0
    for m, layers in ((1024, [1024, 4096, 1024]), (256, [1024, 4096, 1024]), (2048, [1024, 2048, 1024]), (1024, [1024, 2048, 1024, 2048, 1024])):
        assert pick(m, layers)["tile"] == -1 and pick(m, layers)["why"].startswith("gate: "), (m, layers)
    assert pick(1024, [1024, 512, 256, 128], cus=64)["tile"] == -1 and pick(1024, [1024, 512, 256, 128], cus=304)["tile"] == 0
    assert pick(1024, [1024, 512, 256, 128], vf=0)["tile"] == 0 and pick(1024, [1024, 512, 256, 128], vf=4)["tile"] == 0
    # the GPU test's chains: every tile and image forced, taken on that tile (a forced tile is not gated)
    for t, (bm, bn) in enumerate(TILE):
        for vf, base in ((2, 20), (0, 24), (4, 28)):
            mine = [r for r in rows if r["forced"] == base + t and r["m"] == 2 * bm and r["vf"] == vf and not r["strict"]]
            assert len(mine) == 9 and all(r["tile"] == t and r["pt"] == t for r in mine), (t, vf, [r["line"] for r in mine])
            assert any(len(r["ns"]) == 8 for r in mine) and any(r["brs"] == [2, 2, 2] for r in mine) and any(r["brs"] == [3, 1] for r in mine)
            assert any(r["ns"] == [3 * bn, bn, 3 * bn] for r in mine) and any(r["ns"] == [bn, 3 * bn, 3 * bn] for r in mine)
    # the GPU test's MLP: taken on the forced 64x64 tile, not with the switch off; on the smallest tile without a forced one
    assert pick(256, [256, 512, 128, 256], forced=21)["tile"] == 1 and pick(256, [256, 512, 128, 256], forced=21, sw=0)["tile"] == -1
    assert pick(256, [256, 512, 128, 256])["tile"] == 0
    # strict mode: the tile all calls were dispatched on, or none
    strict = [r for r in rows if r["strict"]]
    assert {(r["forced"], r["tile"]) for r in strict} == {(21, 1), (-1, -1)}
    assert any(len(r["ns"]) == 8 and r["forced"] == -1 for r in rows) and any(len(r["ns"]) == 9 for r in rows) and any(len(r["ns"]) == 1 for r in rows)


def _others(name, pattern):
    """{(m, n, ks, brs, cus): the rest of the line} of another chain rule's golden table: its lines with every switch as this file's driver sets it"""
    out = {}
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        for l in f:
            m = re.match(r"^(\d+)x(\d+) k([\d,]+) br([\d,]+) bf16 vf2 " + pattern, l.rstrip("\n"))
            if m:
                out[(int(m.group(1)), int(m.group(2)), m.group(3), m.group(4), int(m.group(5)))] = m.groups()[5:]
    return out


def test_the_other_chain_rules_answer_as_their_golden_tables_say(rows):
    edge = _others("gemm_plan_chain_edge.txt", r'f-1 sw1 et-1 st0 cus(\d+) : .* \| tile(-?\d) "([^"]*)"$')
    rounds = _others("gemm_plan_chain_rounds.txt", r'f-1,-1 sw1 st0 cus(\d+) : \S+ pt-?\d \| tile(-?\d) G(\d+) R\d+ g([01]) "([^"]*)"$')
    ragged = _others("gemm_plan_chain_ragged.txt", r'f-1 sw1 ce1 cr1 et-1 st0 x0 cus(\d+) : v\d+,-?\d+ gf0 kind0 "" \| tile(-?\d) "([^"]*)"')
    hits = {"edge": 0, "rounds": 0, "ragged": 0}
    for r in rows:
        if r["etile"] is None:
            continue
        key = (r["m"], r["ns"][0], ",".join(map(str, r["ks"])), ",".join(map(str, r["brs"])), r["cus"])
        for name, table, mine in (("edge", edge, (str(r["etile"]), r["ewhy"])), ("rounds", rounds, (str(r["rtile"]), str(r["G"]), str(r["gated"]), r["rwhy"])),
                                  ("ragged", ragged, (str(r["gtile"]), r["gwhy"]))):
            if key in table:
                assert mine == table[key], (name, r["line"], table[key])
                hits[name] += 1
    assert all(v >= 4 for v in hits.values()), hits


def test_the_single_call_table_is_what_it_was():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan.txt"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == "47d83170a9e065ad7cac7e1f262fe123749fee1f26741562852271ccc04fc960"


def test_the_translation_unit_holds_exactly_the_instances_of_its_table_and_no_scratch():
    """brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, SUP, true, FLATB, 9>: the four tiles with the loader waves and ring of the plain chain
    of each, the three B images, one chunk per barrier and - tiles 0 and 1 - two: eighteen, no scratch, at most 256 VGPRs, no AGPRs"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(CSRC, "brgemm_bf16_lw_chain_widths.hip"),
                            "-o", os.path.join(tmp, "k.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = blw_codeobj._parse(r.stderr)
    chain = sorted({(tile, sup) + cfg for mode, multi, tile, b_kind, sup, cfg, dims, sym in blw_codeobj.launch_table()[0] if (mode, multi) == (0, 1)})
    assert [(t[0], t[1]) for t in chain] == [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (3, 1)], chain  # (the plain chain's tiles and chunks per barrier)
    want = ["_ZN3tpp14brgemm_bf16_lwI" + "".join("Li%dE" % a for a in t[2:]) + "Li%dELb1ELi%dELi9EEEvNS_9ChainArgsE" % (t[1], image) for t in chain for image in (0, 2, 4)]
    assert len(want) == 18 and sorted(rep) == sorted(want), (sorted(set(rep) - set(want)), sorted(set(want) - set(rep)))
    assert not {n: x for n, x in rep.items() if x[0] or x[1] > 256 or x[2]}, rep
