"""CPU check of the planner's edge-tile rule (tpp-mlir_amd/csrc/gemm_plan.cpp choose_f32_edge_variant, xsmm_hip_set_edge_tiles):
tests/gemm_plan_edge/driver.cpp steps whole-layer calls - m = BM - 1, BM, BM + 1 and n = BN - 4, BN, BN + 4, BN + 2 around each of the four
tiles, k = 32 / 64 / 96, no batch element, leading dimensions off the 4-float grid, each alignment bit off, a bias row with and without its
16 bytes, the generic kernel forced, bf16, and whole layers ragged one way and both - through plan_gemm and plan_gemm_call at 256 and 64
compute units under modes 0, 1, 6, 7, 9 and 10. One line per call and environment, with the decision under every mode;
tests/golden/gemm_plan_edge.txt is the reviewed record. Whatever the table says, every line must also satisfy the rule as restated
here (eligible / edge_rule below), and a mode that does not apply must leave the mode-0 decision untouched, field by field.
And, compile-only: the four edge instances exist in the gfx950 code object and use no scratch."""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_edge.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

LINE = re.compile(r'^(\d+)x(\d+)x(\d+) br(\d+) (f32|bf16) e(\S*) lda(\d+) ldb(\d+) ldc(\d+) al([01])([01])([01]) f(-?\d+) cus(\d+) : '
                  r'v(\d+) (\S+) t(\d+) s(\d+) g(\d+) "([^"]*)" \|((?: \d+:(?:-|e\d+))+)$')
FIELDS = ("m", "n", "k", "br", "dt", "ep", "lda", "ldb", "ldc", "ab16", "c16", "d16", "forced", "cus", "variant", "launcher", "tile", "split",
          "generic", "text")
MODES = [0, 1, 6, 7, 9, 10]
TILE = {6: (64, 64), 7: (64, 32), 9: (32, 32), 10: (128, 64)}  # GemmVariant -> output tile


def ceil_tiles(m, n, v):
    bm, bn = TILE[v]
    return (-(-m // bm)) * (-(-n // bn)) if m >= bm and n >= bn else 0


def edge_rule(m, n, mode, cus):
    """the tile an eligible call takes (a GemmVariant), None = none: restated from the issue, not from the planner's code. Mode 1 is the
    divisible shapes' rule on ceil-divided tile counts: at least a 64x64 tile per CU -> 64x64, or 128x64 if its rounds x 1.85 are fewer;
    else at least a 64x32 tile per CU -> 64x32, or 32x32 if 0.23 x 1.05 x its rounds < 0.46 x those of 64x32; else 32x32 tiles if they
    are at least twice the 64x64 tiles; else the largest tile that fits"""
    t = {v: ceil_tiles(m, n, v) for v in TILE}
    rounds = lambda tiles: -(-tiles // cus)  # noqa: E731
    if mode in TILE:
        return mode if t[mode] else None
    assert mode == 1
    if t[6] >= cus:
        return 10 if t[10] and 1.85 * rounds(t[10]) < rounds(t[6]) else 6
    if t[7] >= cus:
        return 9 if t[9] and 0.23 * 1.05 * rounds(t[9]) < 0.46 * rounds(t[7]) else 7
    if t[9] and t[9] >= 2 * t[6] and t[7] < cus:
        return 9
    for v in (6, 7, 9):
        if t[v]:
            return v
    return None


def eligible(r):
    """everything but the tile: f32, planned on the generic kernel without having been forced there, 64-k chunks and a batch element,
    16-byte pieces of every operand"""
    return (r["dt"] == "f32" and r["variant"] == 8 and r["forced"] != 8 and r["k"] % 64 == 0 and r["br"] >= 1 and r["n"] % 4 == 0 and
            all(r[x] % 4 == 0 and r[x] < 1 << 22 for x in ("lda", "ldb", "ldc")) and r["ab16"] and r["c16"] and ("B" not in r["ep"] or r["d16"]))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_edge")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_edge", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_edge")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    """one row per line and mode. The driver prints a mode's decision as "-" only if every field of the launch and the descriptor's variant
    and name equal the mode-0 decision of the line and it is no edge launch, as "e<variant>" only for launcher f32_lw on that variant's
    tile index with split 1, no tail and the tile's "edge tiles" text, and anything else in full behind a "!" - which LINE does not match"""
    out = []
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "a decision that is neither today's nor an edge launch: " + l
        base = dict(zip(FIELDS, m.groups()[:20]))
        for k in FIELDS:
            if k not in ("dt", "ep", "launcher", "text"):
                base[k] = int(base[k])
        modes = [x.split(":") for x in m.group(21).split()]
        assert [int(a) for a, _ in modes] == MODES, l
        for mode, dec in modes:
            out.append(dict(base, mode=int(mode), line=l, edge=None if dec == "-" else int(dec[1:])))
    return out


def test_planner_reproduces_the_golden_edge_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's edge-tile choices differ from tests/golden/gemm_plan_edge.txt:\n" + diff)


def test_case_list_covers_what_the_rule_depends_on(rows):
    assert {r["cus"] for r in rows} == {256, 64}
    assert {r["mode"] for r in rows} == set(MODES)
    shapes = {(r["m"], r["n"]) for r in rows if r["k"] == 64 and r["br"] == 1}
    for bm, bn in TILE.values():
        assert {(bm + dm, bn + dn) for dm in (-1, 0, 1) for dn in (-4, 0, 4, 2)} <= shapes
    assert {r["k"] for r in rows} >= {32, 64, 96} and any(r["br"] == 0 for r in rows)
    assert any(r["ldc"] % 4 for r in rows) and any(r["lda"] % 4 for r in rows) and any(r["ldb"] % 4 for r in rows)
    assert any(not r["ab16"] for r in rows) and any(not r["c16"] for r in rows)
    assert {("B" in r["ep"], r["d16"]) for r in rows} == {(False, 1), (False, 0), (True, 1), (True, 0)}
    assert any(r["forced"] == 8 for r in rows) and any(r["dt"] == "bf16" for r in rows)
    assert {r["edge"] for r in rows if r["mode"] == 1} >= {6, 7, 9, 10}, "mode 1 reaches every tile"
    # calls that mode 0 runs on the loader-wave 32x32 tile with a ragged n (m a multiple of 32): edge tiles take them too
    assert any(r["launcher"] == "f32_lw_grouped" and r["edge"] for r in rows)
    # the divisible control
    assert all(r["edge"] is None for r in rows if (r["m"], r["n"]) == (1408, 1024))


def test_every_line_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        want = edge_rule(r["m"], r["n"], r["mode"], r["cus"]) if r["mode"] and eligible(r) else None
        assert r["edge"] == want, (r["mode"], want, r["line"])
        if r["edge"]:
            chosen += 1
            bm, bn = TILE[r["edge"]]
            assert r["m"] >= bm and r["n"] >= bn and (r["m"] % 32 or r["n"] % 32), r["line"]
    assert chosen > 100


def test_the_named_shapes_get_the_expected_tile(rows):
    def pick(m, n, br, cus=256):
        got = {r["edge"] for r in rows if (r["m"], r["n"], r["k"], r["br"], r["cus"], r["mode"], r["ep"], r["forced"]) == (m, n, 64, br, cus, 1, "b", -1)
               and r["ldc"] == n and r["ab16"] and r["c16"]}
        assert len(got) == 1, (m, n, br, got)
        return got.pop()
    assert pick(1000, 1000, 1) == pick(1000, 1000, 16) == 6    # 16 x 16 = 256 tiles of 64x64: one round
    assert pick(200, 1000, 1) == 9                             # 7 x 32 = 224 tiles of 32x32 before 4 x 16 of 64x64
    assert pick(4000, 520, 1) == 6                             # 63 x 9 = 567 tiles of 64x64 in 3 rounds; 128x64: 2 x 1.85
    assert pick(2000, 1000, 8) == 10                           # 512 tiles of 64x64 in 2 rounds against 256 of 128x64 in one
    assert pick(65, 68, 16) == 9
    assert pick(1000, 1000, 1, cus=64) == 10


def test_edge_instances_exist_and_use_no_scratch():
    """brgemm_f32_lw_edge<WM, WN, WK, NL, NSLOT, NLB>: 64x64 + K2, 64x32 + K4, 32x32 + K4 and 128x64 with the loader waves of the plain
    launch of each tile"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    src = os.path.join(CSRC, "brgemm_f32_lw.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", os.path.join(tmp, "k.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch), (len(names), len(scratch))
    edge = {n: s for n, s in zip(names, scratch) if n.startswith("_ZN3tpp18brgemm_f32_lw_edgeI")}
    for args in ((2, 2, 2, 2, 4, 2), (2, 1, 4, 2, 4, 1), (1, 1, 4, 1, 4, 1), (4, 2, 1, 2, 3, 2)):
        want = "_ZN3tpp18brgemm_f32_lw_edgeI" + "".join("Li%dE" % a for a in args) + "EE"
        assert any(n.startswith(want) for n in edge), (want, sorted(edge))
    assert not {n: s for n, s in edge.items() if s}, edge
