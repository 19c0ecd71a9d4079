"""CPU check of the planner's bf16 edge-tile rule (tpp-mlir_amd/csrc/gemm_plan.cpp choose_bf16_edge_tile, xsmm_hip_set_edge_tiles modes 2 and
20 .. 23): tests/gemm_plan_edge_bf16/driver.cpp steps whole-layer calls - m = BM - 1, BM, BM + 1 and n = BN - 8, BN, BN + 8, BN + 4 around
each of the four tiles, k = 32 / 64 / 96, no batch element, each leading dimension off its grid, each alignment bit off, a bias row with and
without its 8 bytes, the generic kernel and a variant forced, a VNNI C, the three B images, f32 controls, divisible controls and whole
layers ragged one way and both - through plan_gemm and plan_gemm_call at 256 and 64 compute units under modes 0, 1, 2, 6, 20, 21, 22 and
23. One line per call and environment, with the decision under every mode; tests/golden/gemm_plan_edge_bf16.txt is the reviewed record.
Whatever the table says, every line must also satisfy the rule as restated here (eligible / edge_rule below), a mode that does not apply
must leave the mode-0 decision untouched, field by field, and an f32 call must get under mode 2 what it gets under mode 1.
And, compile-only: the eighteen edge instances exist in the gfx950 code object and use no scratch."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_edge_bf16.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

LINE = re.compile(r'^(\d+)x(\d+)x(\d+) br(\d+) (f32|bf16) vf(\d) vc([01]) e(\S*) lda(\d+) ldb(\d+) ldc(\d+) al([01])([01])([01]) f(-?\d+) cus(\d+) : '
                  r'v(\d+) vfd([01]) (\S+) t(\d+) s(\d+) b(\d+) g(\d+) "([^"]*)" \|((?: \d+:(?:-|e\d+))+)$')
FIELDS = ("m", "n", "k", "br", "dt", "vf", "vnni_c", "ep", "lda", "ldb", "ldc", "ab16", "c16", "d8", "forced", "cus", "variant", "variant_forced",
          "launcher", "tile", "split", "b_kind", "generic", "text")
MODES = [0, 1, 2, 6, 20, 21, 22, 23]
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]  # 32x64 + K2, 64x64, 64x128, 128x128: GemmVariant 20 + t (VNNI-2), 24 + t (flat), 28 + t (VNNI-4)
IMAGE_BASE = {2: 20, 0: 24, 4: 28}
# the fitted model of the divisible shapes (profiles/r06_bf16_sweep.txt): a round of workgroups of tile t costs A[t] + B[t] x chunks us
BLW_A, BLW_B = (3.56, 3.75, 4.66, 6.06), (0.098, 0.135, 0.204, 0.236)


def ceil_tiles(m, n, t):
    bm, bn = TILE[t]
    return (-(-m // bm)) * (-(-n // bn)) if m >= bm and n >= bn else 0


def edge_rule(m, n, chunks, mode, cus):
    """the tile index an eligible bf16 call takes, None = none: restated from the issue, not from the planner's code. Modes 20 .. 23: that
    tile if it fits. Mode 2: among the tiles that fit the cheapest by rounds(ceil-divided tiles, CUs) x (A + B x chunks), chunks = br x k /
    64; ties go to the larger tile"""
    fits = [t for t in range(4) if ceil_tiles(m, n, t)]
    if 20 <= mode <= 23:
        return mode - 20 if mode - 20 in fits else None
    assert mode == 2
    cost = lambda t: -(-ceil_tiles(m, n, t) // cus) * (BLW_A[t] + BLW_B[t] * chunks)  # noqa: E731
    return min(fits, key=lambda t: (cost(t), -t)) if fits else None


def eligible(r):
    """everything but the tile. bf16 without a VNNI C, planned on the generic or the 32x32 K-split kernel without having been forced
    there, no loader-wave tile divides the shape, 64-k chunks and a batch element, n in 16-byte pieces, the image's leading dimensions
    and lane offsets, A / B / C on 16 bytes and a bias row on 8"""
    ldb_ok = {2: r["ldb"] % 4 == 0 and r["ldb"] < 1 << 21, 0: r["ldb"] % 8 == 0 and r["ldb"] < 1 << 21, 4: r["ldb"] % 2 == 0 and r["ldb"] < 1 << 20}
    stride_a, stride_b = r["k"], r["k"] * r["ldb"]  # the driver's layers
    return (r["dt"] == "bf16" and not r["vnni_c"] and r["forced"] != 8 and not r["variant_forced"] and r["variant"] in (8, 19) and
            (r["m"] % 32 != 0 or r["n"] % 64 != 0) and r["k"] > 0 and r["k"] % 64 == 0 and r["br"] >= 1 and r["n"] % 8 == 0 and
            all(r[x] % 8 == 0 and r[x] < 1 << 22 for x in ("lda", "ldc")) and stride_a % 8 == 0 and stride_b % 8 == 0 and ldb_ok[r["vf"]] and
            r["ab16"] and r["c16"] and ("B" not in r["ep"] or r["d8"]))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_edge_bf16")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_edge_bf16", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_edge_bf16")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    """one row per line and mode. The driver prints a mode's decision as "-" only if every field of the launch and the descriptor's variant,
    name and forced flags equal the mode-0 decision of the line and it is no edge launch, as "e<variant>" only for the launcher, tile
    index and B image of that variant number with split 1, no tail and the tile's "edge tiles" text, and anything else in full behind a
    "!" - which LINE does not match"""
    out = []
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "a decision that is neither today's nor an edge launch: " + l
        base = dict(zip(FIELDS, m.groups()[:24]))
        for k in FIELDS:
            if k not in ("dt", "ep", "launcher", "text"):
                base[k] = int(base[k])
        modes = [x.split(":") for x in m.group(25).split()]
        assert [int(a) for a, _ in modes] == MODES, l
        for mode, dec in modes:
            out.append(dict(base, mode=int(mode), line=l, edge=None if dec == "-" else int(dec[1:])))
    return out


def test_planner_reproduces_the_golden_bf16_edge_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's bf16 edge-tile choices differ from tests/golden/gemm_plan_edge_bf16.txt:\n" + diff)


def test_case_list_covers_what_the_rule_depends_on(rows):
    bf = [r for r in rows if r["dt"] == "bf16"]
    assert {r["cus"] for r in rows} == {256, 64}
    assert {r["mode"] for r in rows} == set(MODES)
    shapes = {(r["m"], r["n"]) for r in bf if r["k"] == 64 and r["br"] == 1 and r["vf"] == 2}
    for bm, bn in TILE:
        assert {(bm + dm, bn + dn) for dm in (-1, 0, 1) for dn in (-8, 0, 8, 4)} <= shapes
    assert {r["k"] for r in bf} >= {32, 64, 96} and any(r["br"] == 0 for r in bf)
    for vf, grid in ((2, 4), (0, 8), (4, 2)):
        assert any(r["vf"] == vf and r["ldb"] % grid for r in bf) and any(r["vf"] == vf and r["lda"] % 8 for r in bf)
        assert any(r["vf"] == vf and r["ldc"] % 8 for r in bf) and any(r["vf"] == vf and r["ldc"] != r["n"] and r["edge"] for r in bf)
    assert any(not r["ab16"] for r in bf) and any(not r["c16"] for r in bf)
    assert {("B" in r["ep"], r["d8"]) for r in bf} == {(False, 1), (False, 0), (True, 1), (True, 0)}
    assert any(r["forced"] == 8 for r in bf) and any(r["variant_forced"] for r in bf) and any(r["forced"] == 21 and not r["variant_forced"] for r in bf)
    assert any(r["vnni_c"] for r in bf) and any(r["dt"] == "f32" for r in rows)
    assert any(r["variant"] == 19 and r["edge"] for r in bf), "a call planned on the 32x32 K-split kernel takes edge tiles"
    assert {r["edge"] for r in bf if r["mode"] == 2} >= {20, 21, 22, 23, 24, 27, 28, 31}, "mode 2 reaches every tile and every image"
    for shape in ((1024, 1024), (96, 128), (4096, 1024)):  # the divisible controls
        assert [r for r in rows if (r["m"], r["n"]) == shape] and all(r["edge"] is None for r in rows if (r["m"], r["n"]) == shape)
    assert {(1000, 1000), (200, 1000), (4100, 1024), (1000, 1024)} <= {(r["m"], r["n"]) for r in bf if r["edge"]}


def test_every_line_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        if r["dt"] != "bf16":
            continue
        want = None
        if r["mode"] in (2, 20, 21, 22, 23) and eligible(r):
            t = edge_rule(r["m"], r["n"], r["br"] * r["k"] // 64, r["mode"], r["cus"])
            want = None if t is None else IMAGE_BASE[r["vf"]] + t
        assert r["edge"] == want, (r["mode"], want, r["line"])
        if r["edge"]:
            chosen += 1
            bm, bn = TILE[r["edge"] & 3]
            assert r["m"] >= bm and r["n"] >= bn and (r["m"] % 32 or r["n"] % 64) and r["n"] % 8 == 0, r["line"]
    assert chosen > 300


def test_modes_1_and_6_leave_bf16_alone_and_f32_under_mode_2_is_mode_1(rows):
    assert all(r["edge"] is None for r in rows if r["dt"] == "bf16" and r["mode"] in (0, 1, 6))
    f32 = [r for r in rows if r["dt"] == "f32"]
    by = {(r["line"], r["mode"]): r["edge"] for r in f32}
    assert f32 and any(r["edge"] for r in f32 if r["mode"] == 1)
    for (line, mode), edge in by.items():
        if mode == 2:
            assert edge == by[(line, 1)], line
        if mode >= 20 or mode == 0:
            assert edge is None, line


def test_the_named_shapes_get_the_expected_tile(rows):
    def pick(m, n, br, cus=256, vf=2):
        got = {r["edge"] for r in rows if (r["m"], r["n"], r["k"], r["br"], r["cus"], r["mode"], r["ep"], r["forced"], r["vf"], r["dt"]) ==
               (m, n, 64, br, cus, 2, "b", -1, vf, "bf16") and r["ldc"] == n and r["ab16"] and r["c16"]}
        assert len(got) == 1, (m, n, br, got)
        return got.pop()
    # K = 1024 (16 chunks). 1000 x 1000: 64 tiles of 128x128 - one round, 9.8 us by the model - against 128 of 64x128 (7.9), 256 of 64x64
    # (5.9) and 512 of 32x64 in two rounds (10.3)
    assert pick(1000, 1000, 16) == 21 and pick(1000, 1000, 16, vf=0) == 25 and pick(1000, 1000, 16, vf=4) == 29
    assert pick(200, 1000, 16) == 20          # 112 tiles of 32x64 (5.1 us) before 64 of 64x64 (5.9)
    assert pick(4100, 1024, 16) == 23         # 33 x 8 = 264 tiles of 128x128 in two rounds (19.7) against 520 of 64x128 in three (23.8)
    assert pick(1000, 1024, 16) == 21
    assert pick(72, 72, 16) == 20             # 3 x 2 tiles of 32x64 against 2 x 2 of 64x64: one round each, the cheaper round
    assert pick(1000, 1000, 16, cus=64) == 23


def test_edge_instances_exist_and_use_no_scratch():
    """brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, SUP, false, FLATB, 3>: the four tiles with the loader waves and ring of the
    plain launch of each, both chunks-per-barrier instances of 32x64 + K2 and 64x64, the three B images"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    src = os.path.join(CSRC, "brgemm_bf16_lw.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "k.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs), (len(names), len(scratch), len(vgprs))
    edge = {n: (s, v) for n, s, v in zip(names, scratch, vgprs) if n.startswith("_ZN3tpp14brgemm_bf16_lwI") and n.endswith("Li3EEEvNS_9ChainArgsE")}
    tiles = ((1, 2, 2, 1, 1, 8, 1, 2, 1), (1, 2, 2, 1, 1, 8, 1, 2, 2), (2, 2, 1, 1, 1, 8, 1, 1, 1), (2, 2, 1, 1, 1, 8, 1, 1, 2), (2, 2, 1, 1, 2, 6, 1, 2, 1),
             (2, 2, 1, 2, 2, 4, 1, 1, 1))
    for args in tiles:
        for image in (0, 2, 4):
            want = "_ZN3tpp14brgemm_bf16_lwI" + "".join("Li%dE" % a for a in args) + "Lb0ELi%dELi3EEEvNS_9ChainArgsE" % image
            assert want in edge, (want, sorted(edge))
    assert len(edge) == 18, sorted(edge)
    assert not {n: x for n, x in edge.items() if x[0] or x[1] > 256}, edge
