"""CPU check of the planner's rule for layer chains on the 256x256 bf16 tile (tpp-mlir_amd/csrc/gemm_plan.cpp chain_dma256_b_kind /
chain_dma256_on_tile / plan_chain_dma256, xsmm_hip_set_chain_dma256): tests/gemm_plan_chain_dma256/driver.cpp, compiled with the library's
flags, steps layer chains - every shape of the GPU test under its mode, the three B images, mode 1 on calls forced onto the tile, taken by
xsmm_hip_set_dma256_images and planned by rule, the real overflow, the rows of the A/B in every mode, forced G, strict mode, and one
refusal each - through the rule at 256 and 64 compute units. One line per chain and CU count; tests/golden/gemm_plan_chain_dma256.txt is
the reviewed record. Whatever the table says, every line must also satisfy the rule as restated here from its issue."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_chain_dma256.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

LINE = re.compile(r'^(\d+)x(\d+) k([\d,]+) br([\d,]+) (f32|bf16) vf(\d) f(-?\d+),(-?\d+) img(\d) sw(\d+) st([01]) cus(\d+) : v(\d+),(-?\d+) kind(-?\d) on([01]) \| '
                  r'take([01]) G(\d+) R(\d+) g([01]) "([^"]*)"$')
V_DMA256 = 18


def gate(tiles_m, tiles_n, groups):
    """the measured gate of mode 1 (profiles/chain_dma256_ab.txt), restated: see gemm_plan.h plan_chain_dma256"""
    return GATE(tiles_m, tiles_n, groups)


def GATE(tiles_m, tiles_n, groups):
    """sixteen column tiles (4096 rows x 4096-wide layers) ran slower as one launch in every pair, four (1024-wide) faster: more than eight
    are gated"""
    return tiles_n > 8


def rule(m, n, ks, brs, cus, on_tile, kind, mode, strict):
    """G of the launch, None = not taken - restated from the issue"""
    forced = mode > 1000
    if mode not in (1, 2) and not forced:
        return None
    if kind not in (0, 2, 4) or not 2 <= len(ks) <= 8 or m % 256 or n % 256 or any(k < 32 or k % 32 for k in ks) or any(b < 1 for b in brs):
        return None
    tiles_m, tiles_n = m // 256, n // 256
    gmax = cus // tiles_n
    if gmax == 0 or (strict and not on_tile):
        return None
    if forced:
        g = mode - 1000
        return g if 1 <= g <= tiles_m and g * tiles_n <= cus else None
    if mode == 1 and not on_tile:
        return None
    if tiles_m <= gmax:
        return tiles_m
    r = -(-tiles_m // gmax)
    return -(-tiles_m // r)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_chain_dma256")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_chain_dma256", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_chain_dma256")
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
                        forced0=int(g[6]), forced=int(g[7]), img=int(g[8]), sw=int(g[9]), strict=int(g[10]), cus=int(g[11]), v0=int(g[12]), v1=int(g[13]),
                        kind=int(g[14]), on=int(g[15]), take=int(g[16]), G=int(g[17]), R=int(g[18]), gated=int(g[19]), why=g[20], line=l))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's choices differ from tests/golden/gemm_plan_chain_dma256.txt:\n" + diff)


def test_every_line_keeps_the_rule(rows):
    taken = 0
    for r in rows:
        if r["why"].startswith("the calls differ in m or n"):
            assert not r["take"], r["line"]
            continue
        if r["dt"] == "f32":
            assert r["kind"] == -2, r["line"]
        want = rule(r["m"], r["n"], r["ks"], r["brs"], r["cus"], bool(r["on"]), r["kind"], r["sw"], bool(r["strict"]))
        assert (r["take"], r["G"]) == ((0, 0) if want is None else (1, want)), (want, r["line"])
        assert (r["take"] and not r["gated"]) == (r["why"] == ""), r["line"]
        assert not r["gated"] or (r["sw"] == 1 and r["why"].startswith("gate:")), r["line"]
        if r["take"]:
            taken += 1
            tiles_m, tiles_n = r["m"] // 256, r["n"] // 256
            assert 1 <= r["G"] <= tiles_m and r["G"] * tiles_n <= r["cus"] and r["R"] == -(-tiles_m // r["G"]), r["line"]
            assert r["gated"] == (1 if r["sw"] == 1 and gate(tiles_m, tiles_n, r["G"]) else 0), r["line"]
            if r["sw"] in (1, 2):
                assert r["R"] == -(-tiles_m // min(tiles_m, r["cus"] // tiles_n)), ("as few rounds as fit", r["line"])
            if r["sw"] == 1 or r["strict"]:
                assert r["on"], r["line"]
        else:
            assert (r["G"], r["R"], r["gated"]) == (0, 0, 0), r["line"]
    assert taken > 60


def test_case_list_covers_what_the_issue_names(rows):
    assert {r["cus"] for r in rows} >= {256, 64}

    def pick(m, cus=256, n=1024, sw=1, **kw):
        want = dict(dt="bf16", vf=2, forced0=-1, forced=-1, img=0, strict=0, ks=[n, n, n], brs=[1, 1, 1])
        want.update(kw)
        got = [r for r in rows if (r["m"], r["n"], r["cus"], r["sw"]) == (m, n, cus, sw) and all(r[k] == v for k, v in want.items())]
        assert len(got) == 1, (m, cus, n, sw, kw, len(got))
        return got[0]
    # three 1024-wide layers at 256 CUs: 16384 rows are one round of 64 groups, 32768 rows two rounds, 8192 rows half the chip
    assert (pick(16384)["take"], pick(16384)["G"], pick(16384)["R"], pick(16384)["on"]) == (1, 64, 1, 1)
    assert (pick(32768)["G"], pick(32768)["R"]) == (64, 2)
    assert (pick(4096, n=4096)["G"], pick(4096, n=4096)["R"], pick(4096, n=4096)["on"]) == (16, 1, 1)
    # the gate: 16 column tiles measured slower - mode 1 names the plan and does not launch; mode 2 is not gated; 4 column tiles are not
    assert pick(4096, n=4096)["gated"] == 1 and pick(4096, n=4096, sw=2)["gated"] == 0 and pick(4096, n=4096, sw=2)["take"] == 1
    assert pick(16384)["gated"] == 0 and pick(32768)["gated"] == 0
    # 8192 rows (128 tiles) are not planned on this tile: mode 1 leaves them, mode 2 takes them
    assert pick(8192)["on"] == 0 and not pick(8192)["take"] and pick(8192)["why"].startswith("by rule only where every call runs on the 256x256 tile")
    assert (pick(8192, sw=2)["take"], pick(8192, sw=2)["G"], pick(8192, sw=2)["R"]) == (1, 32, 1)
    assert pick(16384, sw=0)["why"].startswith("chains on the 256x256 tile are off")
    assert pick(16384, sw=3)["why"] == pick(16384, sw=1000)["why"] == pick(16384, sw=0)["why"]
    # at 64 CUs: 16 groups of 4
    assert [(pick(m, cus=64, sw=2)["G"], pick(m, cus=64, sw=2)["R"]) for m in (16384, 4096)] == [(16, 4), (16, 1)]
    # forced G
    assert [(pick(16384, sw=s)["take"], pick(16384, sw=s)["G"], pick(16384, sw=s)["R"]) for s in (1032, 1064, 1065, 1001)] == [(1, 32, 2), (1, 64, 1), (0, 0, 0), (1, 1, 64)]
    assert pick(16384, sw=1065)["why"].startswith("the forced row groups do not fit")
    assert not pick(16384, sw=1032)["gated"], "a forced G is not gated"
    # flat and VNNI-4: mode 1 needs xsmm_hip_set_dma256_images, whose rule takes 16384 rows and not 4096
    for vf in (0, 4):
        assert [pick(16384, vf=vf, img=i)["on"] for i in (0, 1, 2)] == [0, 1, 1] and [pick(4096, vf=vf, img=i)["on"] for i in (0, 1, 2)] == [0, 0, 1]
        assert pick(16384, vf=vf, img=1)["take"] and pick(16384, vf=vf, img=1)["kind"] == {0: 2, 4: 4}[vf]
    # the GPU test's shapes
    for vf in (2, 0, 4):
        for (m, n, k0, br0, sw, want) in ((256, 256, 32, 1, 2, (1, 1, 1)), (512, 512, 96, 1, 2, (1, 2, 1)), (768, 512, 160, 2, 2, (1, 3, 1)), (1024, 512, 224, 1, 2, (1, 4, 1)),
                                          (1280, 256, 32, 1, 1002, (1, 2, 3)), (1024, 512, 96, 1, 1002, (1, 2, 2)), (768, 256, 160, 1, 1001, (1, 1, 3)), (768, 256, 160, 1, 1004, (0, 0, 0))):
            r = pick(m, n=n, sw=sw, vf=vf, ks=[k0, n, n], brs=[br0, 1, 1])
            assert (r["take"], r["G"], r["R"]) == want and r["kind"] == {2: 0, 0: 2, 4: 4}[vf], r["line"]
        f, img = (V_DMA256, 0) if vf == 2 else (-1, 2)
        r = pick(1024, n=512, vf=vf, forced0=f, forced=f, img=img)
        assert (r["take"], r["G"], r["R"], r["on"]) == (1, 4, 1, 1), r["line"]
        assert not pick(1024, n=512, vf=vf)["take"] and not pick(1024, n=512, vf=vf)["on"], "planned by rule, 8 tiles go elsewhere"
        assert not pick(1024, n=512, vf=vf, img=1)["take"]
    # mode 1 on a real overflow: 256 x (CUs + 8) rows of 256 columns make R = 2 at every CU count
    for cus in (256, 64, 304):
        r = pick(256 * (cus + 8), cus=cus, n=256, forced0=V_DMA256, forced=V_DMA256, ks=[64, 256], brs=[1, 1])
        assert (r["take"], r["R"], r["G"]) == (1, 2, (cus + 8 + 1) // 2), r["line"]
    # strict mode
    assert pick(16384, strict=1)["take"], "every call was dispatched on the tile: the separate calls' bits"
    assert pick(4096, sw=2, strict=1)["why"].startswith("strict mode") and pick(4096, sw=1016, strict=1)["why"].startswith("strict mode")
    assert pick(4096, sw=2, strict=1, forced0=V_DMA256, forced=V_DMA256)["take"]
    # one refusal row each
    assert pick(16400, sw=2)["why"] == pick(384, n=256, sw=2)["why"] == pick(512, n=384, sw=2)["why"] == "256 does not divide a chain's m and n"
    for k0 in (40, 1000, 48):
        assert not pick(16384, sw=2, ks=[k0, 1024, 1024])["take"]
    assert pick(16384, sw=2, dt="f32", vf=0)["why"].endswith("an f32 call")
    assert pick(16384, sw=2, ks=[1024], brs=[1])["why"] == pick(16384, sw=2, ks=[1024] * 9, brs=[1] * 9)["why"] == "fewer than 2 or more than 8 calls"
    assert pick(16384, sw=2, ks=[1024] * 8, brs=[1] * 8)["take"]
    assert "empty batch" in pick(16384, sw=2, brs=[0, 1, 1])["why"]
    assert pick(1024, sw=2, ks=[1024, 1024, 512])["why"].startswith("the calls differ in m or n")
    assert pick(16384, sw=2, forced=8)["kind"] == -1 and pick(16384, sw=2, forced=8)["why"].startswith("the calls of a chain on the 256x256 tile share no B image")
    assert pick(256, cus=64, n=32768, sw=2)["why"] == "a row of tiles is wider than the compute units"
