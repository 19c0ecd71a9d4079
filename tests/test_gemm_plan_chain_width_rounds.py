"""CPU check of the planner's column-round rule for mixed-width chains (tpp-mlir_amd/csrc/gemm_plan.cpp plan_chain_width_rounds,
xsmm_hip_set_chain_width_rounds): tests/gemm_plan_chain_width_rounds/driver.cpp, compiled with the library's flags, steps layer chains - the
rows of the A/B at 256, 64 and 304 compute units with xsmm_hip_set_chain_widths off and on, forced W that fit and that do not, the GPU
test's chains with every tile forced and the three B images, strict mode, and one refusal each - through the rule the way try_chain_launch
asks it. One line per chain and CU count; tests/golden/gemm_plan_chain_width_rounds.txt is the reviewed record. Whatever the table says,
every line must also satisfy the rule as restated here from its issue, and every refusal is reached."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_chain_width_rounds.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

LINE = re.compile(r'^(\d+) n([\d,]+) k([\d,]+) br([\d,]+) (f32|bf16) vf(\d) f(-?\d+) sw(\d+) cw([01]) st([01]) x(\d+) cus(\d+) : pt(-?\d) kind(-?\d) \| tile(-?\d) W(\d+) g([01]) "([^"]*)"'
                  r' \| widths tile(-?\d) \| (rounds|widths|none)$')
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]
BLW_B = [0.098, 0.135, 0.204, 0.236]  # gemm_plan.cpp: the fitted time per 64-k chunk of tiles 0 .. 3, us
WHYS = ["column rounds of mixed-width chains are off", "an f32 call", "fewer than 2 or more than 8 calls", "do not share one B image", "k not in 64-k chunks", "an empty batch",
        "every call has the same n", "strict mode", "no tile divides m and every n", "more row blocks than compute units", "the forced column groups do not fit", "gate: "]


def balanced(max_t, tiles_m, cus):
    wfit = min(max_t - 1, cus // tiles_m)
    if wfit < 1:
        return 0
    r = -(-max_t // wfit)
    return -(-max_t // r)


def rounds_rule(m, ns, ks, brs, cus, kind, pt, strict=False, sw=1):
    """(tile, W, gated) of a chain in column rounds, None = refused - restated from the issue. 2 .. 8 bf16 calls with one B image, every
    k >= 64 and a multiple of 64, every batch >= 1, at least two n differ. A tile fits with W when BM divides m, BN divides every n,
    1 <= W < max T and m / BM * W <= CUs. Mode 1: the planned tile if it fits with its balanced W; else never in strict mode, of the tiles
    that fit with their balanced W the smallest sum_l ceil(T_l / W) * BLW_B * br_l * k_l / 64, ties to the larger tile - gated (measured)
    wherever the tile is not the planned one. Mode 1000 + W: that W on the planned tile, without one on the
    smallest tile that fits with it; never gated."""
    if not (sw == 1 or sw > 1000) or pt < -1 or not 2 <= len(ns) <= 8 or kind not in (0, 2, 4) or any(k < 64 or k % 64 for k in ks) or any(b < 1 for b in brs) or len(set(ns)) == 1:
        return None
    divides = lambda t: m % TILE[t][0] == 0 and all(n % TILE[t][1] == 0 for n in ns)
    fit = lambda t, w: divides(t) and 1 <= w < max(ns) // TILE[t][1] and (m // TILE[t][0]) * w <= cus
    bal = lambda t: balanced(max(ns) // TILE[t][1], m // TILE[t][0], cus)
    if pt < 0 and strict:
        return None
    if sw > 1000:
        w = sw - 1000
        cand = [pt] if pt >= 0 else list(range(4))
        tiles = [t for t in cand if fit(t, w)]
        return (tiles[0], w, False) if tiles else None
    if pt >= 0 and divides(pt) and fit(pt, bal(pt)):
        return (pt, bal(pt), False)
    if strict:
        return None
    best = None
    for t in range(4):
        if divides(t) and fit(t, bal(t)):
            cost = sum(-(-(n // TILE[t][1]) // bal(t)) * BLW_B[t] * b * (k // 64) for n, k, b in zip(ns, ks, brs))
            if best is None or cost <= best[0]:
                best = (cost, t)
    if best is None:
        return None
    return (best[1], bal(best[1]), True)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_chain_width_rounds")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_chain_width_rounds", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_chain_width_rounds")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    out = []
    names = "m ns ks brs dt vf forced sw cw strict extra cus pt kind tile W gated why wtile launch".split()
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "unreadable line: " + l
        r = dict(zip(names, m.groups()))
        for k in r:
            if k in ("ns", "ks", "brs"):
                r[k] = [int(x) for x in r[k].split(",")]
            elif k not in ("dt", "why", "launch"):
                r[k] = int(r[k])
        r["line"] = l
        out.append(r)
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's column-round choices differ from tests/golden/gemm_plan_chain_width_rounds.txt:\n" + diff)


def test_every_line_keeps_the_rule(rows):
    chosen = gated = 0
    for r in rows:
        want = rounds_rule(r["m"], r["ns"], r["ks"], r["brs"], r["cus"], r["kind"], r["pt"], bool(r["strict"]), r["sw"])
        assert (r["tile"], r["W"], bool(r["gated"])) == ((-1, 0, False) if want is None else want), (want, r["line"])
        assert (r["tile"] >= 0 and not r["gated"]) == (r["why"] == ""), r["line"]
        if r["tile"] >= 0:
            chosen += 1
            gated += r["gated"]
            bm, bn = TILE[r["tile"]]
            assert r["m"] % bm == 0 and all(n % bn == 0 for n in r["ns"]) and 1 <= r["W"] < max(r["ns"]) // bn and (r["m"] // bm) * r["W"] <= r["cus"], r["line"]
            assert r["dt"] == "bf16" and not r["extra"] and len(set(r["ns"])) > 1, r["line"]
            assert not r["gated"] or (r["sw"] == 1 and r["why"].startswith("gate: ") and r["pt"] != r["tile"]), "a forced W and a planned tile are never gated: " + r["line"]
        if r["kind"] >= 0 and r["extra"] == 0 and r["vf"] in (0, 2, 4) and r["forced"] != 8:
            assert r["dt"] == "bf16"
        # try_chain_launch's order of asking: a forced W, the one-round rule, this rule
        mine = r["tile"] >= 0 and not r["gated"]
        assert r["launch"] == ("rounds" if r["sw"] > 1000 and mine else "widths" if r["wtile"] >= 0 else "rounds" if mine else "none"), r["line"]
        assert r["cw"] or r["wtile"] < 0
    assert chosen > 150 and gated >= 10


def test_every_refusal_is_reached_and_the_case_list_covers_what_the_issue_names(rows):
    for w in WHYS:
        assert any(w in r["why"] for r in rows), w
    assert all(any(w in r["why"] for w in WHYS) for r in rows if r["why"]), "a why the test does not know"
    assert {r["cus"] for r in rows} == {64, 256, 304}

    def pick(m, layers, cus=256, vf=2, forced=-1, sw=1, cw=0, strict=0):
        got = [r for r in rows if (r["m"], r["ns"], r["ks"], r["cus"], r["vf"], r["forced"], r["sw"], r["cw"], r["strict"]) == (m, layers[1:], layers[:-1], cus, vf, forced, sw, cw, strict) and
               all(b == 1 for b in r["brs"]) and r["dt"] == "bf16" and not r["extra"] and r["kind"] >= 0]
        assert got and len({(g["tile"], g["W"]) for g in got}) == 1, (m, layers, cus, len(got))
        return got[0]
    ffn = [1024, 4096, 1024]
    # the issue's spot checks, 256 CUs, VNNI-2, no planned tile: tile and W by the fitted rates - and gated, as they measured
    for m, tile, w in ((1024, 1, 16), (4096, 3, 8), (2048, 3, 16)):
        r = pick(m, ffn)
        assert (r["tile"], r["W"], r["gated"], r["launch"]) == (tile, w, 1, "none"), r["line"]
    # (the one-round rule refuses or gates all of them, so this rule is asked with that switch on as well - and gates)
    assert all(pick(m, ffn, cw=1)["wtile"] == -1 and pick(m, ffn, cw=1)["launch"] == "none" for m in (256, 1024, 2048, 4096))
    # the funnel: gated here as well (faster in one session, slower in the next), the one-round launch's with that switch on
    f = [1024, 512, 256, 128]
    assert (pick(1024, f)["tile"], pick(1024, f)["W"], pick(1024, f)["gated"], pick(1024, f)["launch"]) == (0, 4, 1, "none")
    assert pick(1024, f, cw=1)["wtile"] == 0 and pick(1024, f, cw=1)["launch"] == "widths", "a chain the one-round rule takes is not offered here"
    # forced W: fitting - on the smallest tile that fits with it, never gated, in front of the one-round rule - and not
    assert (pick(1024, ffn, sw=1008)["tile"], pick(1024, ffn, sw=1016)["tile"], pick(1024, ffn, sw=1004)["tile"]) == (0, 1, 0)
    assert all(pick(1024, ffn, sw=1000 + w)["gated"] == 0 and pick(1024, ffn, sw=1000 + w, cw=1)["launch"] == "rounds" for w in (4, 8, 16))
    assert pick(1024, ffn, sw=1032)["tile"] == -1 and pick(1024, ffn, sw=1064)["tile"] == -1 and pick(1024, ffn, sw=1300)["tile"] == -1, "8 x 32 = 256 fits only where max T > 32"
    assert (pick(1024, ffn, forced=21, sw=1008)["tile"], pick(1024, ffn, forced=21, sw=1016)["W"]) == (1, 16)
    # the GPU test's chains: every tile and image forced, taken on that tile with the forced W
    for t, (bm, bn) in enumerate(TILE):
        for vf, base in ((2, 20), (0, 24), (4, 28)):
            mine = [r for r in rows if r["forced"] == base + t and r["m"] in (2 * bm, 3 * bm) and r["vf"] == vf and not r["strict"] and r["sw"] in (1001, 1002, 1003)]
            assert len(mine) == 10, (t, vf, [r["line"] for r in mine])
            for r in mine:
                if vf == 2 and r["m"] % 64:  # (the VNNI-2 image of the loader-wave tiles asks for m % 64 == 0: 3 x 32 rows have no image)
                    assert (t, r["m"], r["kind"], r["tile"]) == (0, 96, -1, -1), r["line"]
                else:
                    assert r["tile"] == t and r["pt"] == t and r["W"] == r["sw"] - 1000 and not r["gated"], r["line"]
            assert any(len(r["ns"]) == 8 for r in mine) and any(r["brs"] == [2, 2, 2] for r in mine) and any(r["brs"] == [3, 1] for r in mine) and any(r["m"] == 3 * bm for r in mine)
    # the chain that exceeds the chip: the rule's balanced W on the planned 32x64 tile, not gated; the one-round rule refuses it
    wide = [r for r in rows if r["ns"] == [640, 64, 640]]
    assert {(r["cus"], r["tile"], r["W"], r["gated"]) for r in wide if r["sw"] == 1} == {(256, 0, 5, 0), (64, 0, 2, 0), (304, 0, 5, 0)}
    assert [r["tile"] for r in wide if r["sw"] == 1009] == [-1] and [(r["wtile"], r["launch"]) for r in wide if r["sw"] == 0] == [(-1, "none")]
    # the GPU test's MLP under force_variant(21): mode 1002, off, and by the rule without a forced tile (gated)
    mlp = [256, 512, 128, 256]
    assert (pick(256, mlp, forced=21, sw=1002)["tile"], pick(256, mlp, forced=21, sw=1002)["W"]) == (1, 2) and pick(256, mlp, forced=21, sw=0)["tile"] == -1
    assert pick(256, mlp)["gated"] == 1
    # strict mode: the tile all calls were dispatched on (rule and forced W), or none
    strict = [r for r in rows if r["strict"]]
    assert {(r["forced"], r["sw"], r["tile"]) for r in strict} == {(21, 1002, 1), (21, 1, 1), (-1, 1, -1), (-1, 1002, -1), (20, 1, -1)}
    assert any(r["forced"] == 20 and r["m"] == 16384 and not r["strict"] and r["tile"] > 0 for r in rows), "a planned tile that does not fit: another tile, not in strict mode"
    assert any(len(r["ns"]) == 8 and r["tile"] >= 0 for r in rows) and any(len(r["ns"]) == 9 for r in rows) and any(len(r["ns"]) == 1 for r in rows)
