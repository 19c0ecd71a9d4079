"""CPU check of the planner's ragged-chain rule (tpp-mlir_amd/csrc/gemm_plan.cpp chain_edge_b_kind / plan_chain_edge, xsmm_hip_set_chain_edge):
tests/gemm_plan_chain_edge/driver.cpp, compiled with the library's flags, steps layer chains - the GPU test's shapes around each of the
four tiles with that tile forced, the three B images, the rows of the A/B (1000, 1366, 2000, 4100 and the divisible 1024, 4096 x 1024) with
no tile and with each tile forced, a rank's share of 4096 rows over 6 ranks, and one refusal each: too many tiles, strict mode, the switch
off, the generic kernel forced, a ragged n, m below every tile, f32, a ragged k, an empty batch, one and nine calls - through both
functions at 256 and 64 compute units. One line per chain and CU count; tests/golden/gemm_plan_chain_edge.txt is the reviewed record.
Whatever the table says, every line must also satisfy the rule as restated here from its issue.
And, compile-only: the twelve ragged-chain instances exist in the gfx950 code object and use no scratch."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_chain_edge.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402
import blw_codeobj  # noqa: E402

LINE = re.compile(r'^(\d+)x(\d+) k([\d,]+) br([\d,]+) (f32|bf16) vf(\d) f(-?\d+) sw([01]) et(-?\d) st([01]) cus(\d+) : v(\d+) gf([01]) kind(-?\d) "([^"]*)" \| '
                  r'tile(-?\d) "([^"]*)"$')
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]


def chain_edge_rule(m, n, ks, brs, cus, forced_tile=None, strict=False):
    """the tile a ragged chain takes, None = call by call - restated from the issue. A tile fits when m >= BM, n % BN == 0 and
    ceil(m / BM) * (n / BN) <= CUs; the forced tile if it fits, else the smallest that fits; never in strict mode, with fewer than 2 or more
    than 8 calls, a k that is no multiple of 64 or an empty batch; and a tile whose rows divide m is the divisible chain's business"""
    if strict or not 2 <= len(ks) <= 8 or any(k < 64 or k % 64 for k in ks) or any(b < 1 for b in brs):
        return None
    fits = [t for t, (bm, bn) in enumerate(TILE) if m >= bm and n % bn == 0 and -(-m // bm) * (n // bn) <= cus]
    if not fits:
        return None
    t = forced_tile if forced_tile in fits else fits[0]
    return None if m % TILE[t][0] == 0 else t


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_chain_edge")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_chain_edge", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_chain_edge")
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
                        forced=int(g[6]), sw=int(g[7]), et=int(g[8]), strict=int(g[9]), cus=int(g[10]), variant=int(g[11]), gf=int(g[12]), kind=int(g[13]),
                        kind_why=g[14], tile=int(g[15]), tile_why=g[16], line=l))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's ragged-chain choices differ from tests/golden/gemm_plan_chain_edge.txt:\n" + diff)


def test_every_line_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        want = chain_edge_rule(r["m"], r["n"], r["ks"], r["brs"], r["cus"], r["et"] if r["et"] >= 0 else None, bool(r["strict"]))
        assert r["tile"] == (-1 if want is None else want), (want, r["line"])
        assert (r["tile"] >= 0) == (r["tile_why"] == ""), r["line"]
        if r["tile"] >= 0:
            chosen += 1
            bm, bn = TILE[r["tile"]]
            assert r["m"] >= bm and r["m"] % bm and r["n"] % bn == 0 and -(-r["m"] // bm) * (r["n"] // bn) <= r["cus"], r["line"]
        # a call's B image: none with the switch off, for f32, for a forced kernel, for a k off its chunks; else the image of its B operand
        forced_kernel = r["forced"] == 8 or (r["forced"] >= 0 and r["variant"] == r["forced"])  # (a forced tile the shape does not divide is not honoured)
        eligible = r["sw"] and r["dt"] == "bf16" and not forced_kernel and all(k % 64 == 0 for k in r["ks"])
        assert r["kind"] == ({2: 0, 0: 2, 4: 4}[r["vf"]] if eligible else -1), r["line"]
        assert (r["kind"] >= 0) == (r["kind_why"] == ""), r["line"]
    assert chosen > 100


def test_case_list_covers_what_the_issue_names(rows):
    assert {r["cus"] for r in rows} == {256, 64}
    for t, (bm, bn) in enumerate(TILE):  # the GPU test's shapes, on the tile they force, every B image
        for m in (bm + 8, 3 * bm - 3):
            for n in (bn, 2 * bn):
                got = {(r["vf"], r["tile"]) for r in rows if (r["m"], r["n"], r["et"], r["ks"][0], r["cus"]) == (m, n, t, 192, 256)}
                assert got == {(2, t), (0, t), (4, t)}, (t, m, n, got)
        assert any(r["m"] == 3 * bm - 3 and r["brs"] == [2, 2, 2] and r["tile"] == t for r in rows)
        assert all(r["tile"] == -1 for r in rows if (r["m"], r["n"], r["et"]) == (2 * bm, 2 * bn, t)), "a divisible chain is not this rule's"

    def pick(m, cus=256, n=1024, et=-1, **kw):
        want = dict(dt="bf16", vf=2, forced=-1, sw=1, strict=0)
        want.update(kw)
        got = [r for r in rows if (r["m"], r["n"], r["cus"], r["et"]) == (m, n, cus, et) and r["ks"] == [1024, 1024, 1024] and r["brs"] == [1, 1, 1] and
               all(r[k] == v for k, v in want.items())]
        assert len(got) == 1, (m, cus, n, et, kw, len(got))
        return got[0]
    # 1000 rows: 16 x 16 tiles of 64x64 fill 256 CUs (32 x 16 of 32x64 do not fit); 1366: 22 x 8 of 64x128; 2000: 32 x 8 of 64x128
    assert [pick(m)["tile"] for m in (1000, 1366, 2000)] == [1, 2, 2]
    # 4100 rows need 33 x 8 = 264 tiles of 128x128: one more row of tiles than 256 CUs hold
    assert pick(4100)["tile"] == -1 and pick(4100)["tile_why"] == "more tiles than compute units"
    assert [pick(m, cus=64)["tile"] for m in (1000, 1366, 4100)] == [3, -1, -1]
    assert pick(1000, et=3)["tile"] == 3 and pick(1000, et=0)["tile"] == 1, "a forced tile that fits; one that does not: the smallest that fits"
    assert pick(1024)["tile"] == -1 and pick(4096)["tile"] == -1
    assert pick(4032)["tile"] == 3, "63 x 64 rows: no tile that divides m fits 256 CUs, 32 x 8 shifted tiles of 128x128 do"
    # one refusal row each
    assert pick(8200)["tile_why"] == "more tiles than compute units"
    assert pick(1000, strict=1)["tile_why"].startswith("strict mode")
    assert pick(1000, sw=0)["kind_why"].startswith("ragged chains are off")
    assert pick(1000, forced=8)["kind_why"].endswith("forced kernel") and pick(1000, forced=8)["gf"] == 1
    assert pick(1000, dt="f32", vf=0)["kind_why"].endswith("an f32 call")
    assert pick(1000, n=1032)["tile_why"].endswith("not in whole column tiles")
    assert pick(24)["tile_why"].endswith("below every tile's rows")
    assert any(r["ks"][0] == 1000 and r["kind"] == -1 and r["tile"] == -1 for r in rows), "a ragged k"
    assert {len(r["ks"]) for r in rows} >= {1, 3, 8, 9} and all(r["tile"] == -1 for r in rows if len(r["ks"]) in (1, 9))
    assert any(r["brs"][0] == 0 and r["tile"] == -1 for r in rows)


def test_ragged_chain_instances_exist_and_use_no_scratch():
    """brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, 1, true, FLATB, 5>: the four tiles with the loader waves and ring of the divisible
    chain of each, one chunk per barrier only, the three B images - no scratch, no AGPRs, at most 256 VGPRs"""
    rep = blw_codeobj.report()
    edge = {n: x for n, x in rep.items() if n.endswith("Li5EEEvNS_9ChainArgsE")}
    # the four tiles' configurations as the launch table (brgemm_bf16_lw_launch.h) gives them to the divisible chain, one chunk per barrier
    tiles = sorted({cfg + (1,) for mode, multi, tile, b_kind, sup, cfg, dims, sym in blw_codeobj.launch_table()[0] if (mode, multi) == (0, 1)})
    assert len(tiles) == 4, tiles
    for args in tiles:
        for image in (0, 2, 4):
            want = "_ZN3tpp14brgemm_bf16_lwI" + "".join("Li%dE" % a for a in args) + "Lb1ELi%dELi5EEEvNS_9ChainArgsE" % image
            assert want in edge, (want, sorted(edge))
    assert len(edge) == 12, sorted(edge)
    assert not {n: x for n, x in edge.items() if x[0] or x[1] > 256 or x[2]}, edge
