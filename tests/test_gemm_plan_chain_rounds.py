"""CPU check of the planner's multi-round chain rule (tpp-mlir_amd/csrc/gemm_plan.cpp chain_rounds_planned_tile / plan_chain_rounds,
xsmm_hip_set_chain_rounds): tests/gemm_plan_chain_rounds/driver.cpp, compiled with the library's flags, steps layer chains - every shape of
the GPU test with its tile forced at dispatch and its mode 1000 + G, the three B images, three 1024-wide layers at 4224, 8192, 16384 and
32768 rows and the divisible 1024 and 4096 with the switch on and off, forced G on 8192 rows, and one refusal each: the switch off, strict
mode with mixed tiles, a ragged m, a ragged n, a k % 64, f32, a forced G that does not fit, one and nine calls, an empty batch, a row of
tiles wider than the compute units - through the rule at 256 and 64 compute units. One line per chain and CU count;
tests/golden/gemm_plan_chain_rounds.txt is the reviewed record. Whatever the table says, every line must also satisfy the rule as restated
here from its issue. And, compile-only: the twelve multi-round instances exist in the gfx950 code object, use no scratch and no AGPRs."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_chain_rounds.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402
import blw_codeobj  # noqa: E402

LINE = re.compile(r'^(\d+)x(\d+) k([\d,]+) br([\d,]+) (f32|bf16) vf(\d) f(-?\d+),(-?\d+) sw(\d+) st([01]) cus(\d+) : v(\d+),(-?\d+) pt(-?\d) \| '
                  r'tile(-?\d) G(\d+) R(\d+) g([01]) "([^"]*)"$')
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]
NSLOT = [8, 8, 6, 4]
BASE = {2: 20, 0: 24, 4: 28}


def chain_rounds_rule(m, n, ks, brs, cus, planned_tile, mode, strict):
    """(tile, G) of a multi-round chain, None = not this rule's - restated from the issue. planned_tile: the loader-wave tile all calls
    were planned on, -1 none, -2 an f32 call. The gate (mode 1 only, from the measurement in profiles/chain_rounds_ab.txt: two rounds were
    faster as one launch, four and eight slower) does not change the answer: a chain of more than two rounds is GATED - the line names
    the rule's tile and groups, and the chain stays call by call"""
    forced = mode > 1000
    if mode != 1 and not forced:
        return None
    if planned_tile == -2 or not 2 <= len(ks) <= 8 or any(k < 64 or k % 64 for k in ks) or any(b < 1 for b in brs):
        return None
    divides = [t for t, (bm, bn) in enumerate(TILE) if m >= bm and n >= bn and m % bm == 0 and n % bn == 0]
    if planned_tile >= 0:
        if planned_tile not in divides:
            return None
        t = planned_tile
    elif strict or not divides:
        return None
    else:
        t = divides[-1]  # the largest tile whose rows divide m and whose columns divide n
    tiles_m, tiles_n = m // TILE[t][0], n // TILE[t][1]
    gmax = cus // tiles_n
    if gmax == 0:
        return None
    if forced:
        g = mode - 1000
        return (t, g) if 1 <= g < tiles_m and g * tiles_n <= cus else None
    if tiles_m <= gmax:
        return None  # a chain that fits is today's kernel
    r = -(-tiles_m // gmax)
    return (t, -(-tiles_m // r))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_chain_rounds")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_chain_rounds", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_chain_rounds")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    out = []
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "unreadable line: " + l
        g = m.groups()
        out.append(dict(m=int(g[0]), n=int(g[1]), ks=[int(x) for x in g[2].split(",")], brs=[int(x) for x in g[3].split(",")], dt=g[4], vf=int(g[5]),
                        forced0=int(g[6]), forced=int(g[7]), sw=int(g[8]), strict=int(g[9]), cus=int(g[10]), v0=int(g[11]), v1=int(g[12]), pt=int(g[13]),
                        tile=int(g[14]), G=int(g[15]), R=int(g[16]), gated=int(g[17]), why=g[18], line=l))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's multi-round choices differ from tests/golden/gemm_plan_chain_rounds.txt:\n" + diff)


def test_every_line_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        # the tile all calls were planned on: variants 20 .. 23, 24 .. 27, 28 .. 31 are the four tiles with the three B images
        if r["dt"] == "f32":
            want_pt = -2
        elif 20 <= r["v0"] < 32 and (len(r["ks"]) == 1 or r["v1"] == r["v0"]):
            want_pt = (r["v0"] - 20) % 4
        else:
            want_pt = -1
        assert r["pt"] == want_pt, r["line"]
        want = chain_rounds_rule(r["m"], r["n"], r["ks"], r["brs"], r["cus"], r["pt"], r["sw"], bool(r["strict"]))
        assert (r["tile"], r["G"]) == ((-1, 0) if want is None else want), (want, r["line"])
        assert (r["tile"] >= 0 and not r["gated"]) == (r["why"] == ""), r["line"]
        assert r["gated"] == (1 if want is not None and r["sw"] == 1 and r["R"] > 2 else 0), ("the gate: mode 1, more than two rounds", r["line"])
        assert not r["gated"] or r["why"].startswith("gate:"), r["line"]
        if r["tile"] >= 0:
            chosen += 1
            bm, bn = TILE[r["tile"]]
            tiles_m, tiles_n = r["m"] // bm, r["n"] // bn
            assert r["m"] % bm == 0 and r["n"] % bn == 0 and 1 <= r["G"] <= tiles_m and r["G"] * tiles_n <= r["cus"], r["line"]
            assert r["R"] == -(-tiles_m // r["G"]), r["line"]
            if r["sw"] == 1:
                assert tiles_m * tiles_n > r["cus"] and r["R"] >= 2, ("mode 1 is for chains that do not fit", r["line"])
                assert r["R"] == -(-tiles_m // (r["cus"] // tiles_n)), ("as few rounds as fit", r["line"])
        else:
            assert r["R"] == 0, r["line"]
    assert chosen > 100


def test_case_list_covers_what_the_issue_names(rows):
    assert {r["cus"] for r in rows} >= {256, 64}

    def pick(m, cus=256, n=1024, sw=1, **kw):
        want = dict(dt="bf16", vf=2, forced0=-1, forced=-1, strict=0, ks=[n, n, n], brs=[1, 1, 1])
        want.update(kw)
        got = [r for r in rows if (r["m"], r["n"], r["cus"], r["sw"]) == (m, n, cus, sw) and all(r[k] == v for k, v in want.items())]
        assert len(got) == 1, (m, cus, n, sw, kw, len(got))
        return got[0]
    # three 1024-wide layers at 256 CUs: 8192 rows G = 32, R = 2; 4224 rows (33 x 8 tiles of 128x128) G = 17, R = 2; 32768 rows R = 8
    assert (pick(8192)["tile"], pick(8192)["G"], pick(8192)["R"]) == (3, 32, 2)
    assert (pick(4224)["tile"], pick(4224)["G"], pick(4224)["R"]) == (3, 17, 2)
    assert (pick(32768)["tile"], pick(32768)["G"], pick(32768)["R"]) == (3, 32, 8)
    assert (pick(16384)["G"], pick(16384)["R"]) == (32, 4)
    # .. of which the two-round rows are taken and the rows of four and eight rounds gated (measured slower as one launch)
    assert [pick(m)["gated"] for m in (4224, 8192, 16384, 32768)] == [0, 0, 1, 1]
    assert pick(8192, sw=1016)["gated"] == 0, "a forced G is not gated"
    assert pick(4096)["tile"] == -1 and pick(4096)["why"].startswith("the chain fits in one round"), "4096 rows at 256 CUs are not this rule's"
    assert pick(1024)["tile"] == -1
    # the same shapes at 64 CUs: 8 groups of 8 workgroups
    assert [(pick(m, cus=64)["G"], pick(m, cus=64)["R"]) for m in (8192, 4224, 32768, 4096)] == [(8, 8), (7, 5), (8, 32), (8, 4)]
    # forced G on 8192 rows: 16 groups make 4 rounds; 33 groups of 8 do not fit 256 CUs; G = tiles_m is not several rounds
    assert (pick(8192, sw=1016)["G"], pick(8192, sw=1016)["R"]) == (16, 4) and (pick(8192, sw=1032)["G"], pick(8192, sw=1032)["R"]) == (32, 2)
    assert all(pick(8192, sw=s)["why"].startswith("the forced row groups do not fit") for s in (1033, 1063, 1064))
    assert (pick(4096, sw=1016)["G"], pick(4096, sw=1016)["R"]) == (16, 2), "a forced G also applies to a chain that fits in one round"
    # every GPU-test shape, on the tile it forces, every B image
    for t, (bm, bn) in enumerate(TILE):
        ns = 64 * NSLOT[t]
        for vf in (2, 0, 4):
            f = BASE[vf] + t
            for (m, n, ks, brs, sw, want) in ((5 * bm, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 1002, (t, 2, 3)),
                                             (4 * bm, bn, [192, bn, bn], [1, 1, 1], 1002, (t, 2, 2)),
                                             (3 * bm, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 1001, (t, 1, 3)),
                                             (3 * bm, ns, [ns, ns, ns], [1, 1, 1], 1002, (t, 2, 2)),
                                             (5 * bm, 2 * bn, [128, bn, bn], [2, 2, 2], 1002, (t, 2, 3)),
                                             (3 * bm, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 1003, (-1, 0, 0)),
                                             (3 * bm, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 1, (-1, 0, 0))):
                r = pick(m, n=n, sw=sw, vf=vf, forced0=f, forced=f, ks=ks, brs=brs)
                assert (r["tile"], r["G"], r["R"]) == want and r["v0"] == f and r["pt"] == t, r["line"]
    # mode 1 on a real overflow, tile 0 forced: 32 x (CUs + 8) rows of 64 columns make R = 2 at every CU count
    for cus in (256, 64, 304):
        r = pick(32 * (cus + 8), cus=cus, n=64, forced0=20, forced=20)
        assert (r["tile"], r["R"], r["G"]) == (0, 2, (cus + 8 + 1) // 2), r["line"]
    assert pick(32 * 264, n=64, forced0=20, forced=20, strict=1)["tile"] == 0, "strict mode takes the rule on the planned tile"
    # one refusal row each
    assert pick(8192, sw=0)["why"].startswith("multi-round chains are off")
    mixed = pick(8192, forced0=21)
    assert mixed["v0"] != mixed["v1"] and mixed["tile"] == 3, "mixed tiles: the largest tile that divides"
    assert pick(8192, forced0=21, strict=1)["why"].startswith("strict mode")
    assert pick(8200)["why"].endswith("not in whole tiles") and pick(4100)["why"].endswith("not in whole tiles"), "a ragged m: 4100 rows stay call by call"
    assert pick(8192, n=1032, ks=[1024, 1024, 1024])["why"].endswith("not in whole tiles"), "a ragged n"
    assert pick(8192, ks=[1000, 1024, 1024])["why"].startswith("a layer of a multi-round chain has k not in 64-k chunks")
    assert pick(8192, dt="f32", vf=0)["why"].endswith("an f32 call")
    assert pick(8192, ks=[1024], brs=[1])["why"] == pick(8192, ks=[1024] * 9, brs=[1] * 9)["why"] == "fewer than 2 or more than 8 calls"
    assert pick(8192, ks=[1024] * 8, brs=[1] * 8)["tile"] == 3
    assert pick(8192, brs=[0, 1, 1])["tile"] == -1 and "empty batch" in pick(8192, brs=[0, 1, 1])["why"]
    assert pick(8192, cus=64, n=32768)["why"] == "a row of tiles is wider than the compute units"


def test_multi_round_instances_exist_and_use_no_scratch():
    """brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, 1, true, FLATB, 7>: the four tiles with the loader waves and ring of the divisible
    chain of each, one chunk per barrier only, the three B images - no scratch, no AGPRs, at most 256 VGPRs"""
    rep = blw_codeobj.report()
    rounds = {n: x for n, x in rep.items() if n.endswith("Li7EEEvNS_9ChainArgsE")}
    # the four tiles' configurations as the launch table (brgemm_bf16_lw_launch.h) gives them to the divisible chain, one chunk per barrier
    tiles = sorted({cfg + (1,) for mode, multi, tile, b_kind, sup, cfg, dims, sym in blw_codeobj.launch_table()[0] if (mode, multi) == (0, 1)})
    assert len(tiles) == 4, tiles
    for args in tiles:
        for image in (0, 2, 4):
            want = "_ZN3tpp14brgemm_bf16_lwI" + "".join("Li%dE" % a for a in args) + "Lb1ELi%dELi7EEEvNS_9ChainArgsE" % image
            assert want in rounds, (want, sorted(rounds))
    assert len(rounds) == 12, sorted(rounds)
    assert not {n: x for n, x in rounds.items() if x[0] or x[1] > 256 or x[2]}, rounds
