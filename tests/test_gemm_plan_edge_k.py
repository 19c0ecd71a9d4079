"""CPU check of the planner's ragged-k rule (tpp-mlir_amd/csrc/gemm_plan.cpp plan_gemm_call, xsmm_hip_set_edge_k):
tests/gemm_plan_edge_k/driver.cpp steps whole-layer calls - outputs around each of the four tiles, k below 64, multiples of 64, of 8, of 4
only and odd, 0 / 1 / 3 batch elements, leading dimensions off the 4-float grid, each alignment bit off, a bias row with and without its
16 bytes, forced kernels, bf16, transposed operands, a VNNI C, and whole layers with a ragged K - through plan_gemm and plan_gemm_call
at 256 and 64 compute units under edge_k modes 0, 1, 6, 7, 9, 10 combined with edge-tile modes 0, 1, 2, 6, 10, 21. One line per call and CU
count; tests/golden/gemm_plan_edge_k.txt is the reviewed record. Whatever the table says, every decision must also satisfy the rule as
restated here, and a mode that does not apply must leave the decision of the same edge-tile mode untouched, field by field.
And, compile-only: the four ragged-k instances exist in the gfx950 code object and use no scratch."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_edge_k.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402
from test_gemm_plan_edge import TILE, edge_rule  # noqa: E402  (the tile rule of the edge tiles, restated there from its issue)

HEAD = re.compile(r'^(\d+)x(\d+)x(\d+) br(\d+) (f32|bf16) e(\S*) lda(\d+) ldb(\d+) ldc(\d+) al([01])([01])([01]) f(-?\d+) x([01])([01])([01]) cus(\d+) : '
                  r'v(\d+) (\S+) t(\d+) s(\d+) g(\d+) "([^"]*)"$')
FIELDS = ("m", "n", "k", "br", "dt", "ep", "lda", "ldb", "ldc", "ab16", "c16", "d16", "forced", "a_trans", "b_trans", "vnni_c", "cus", "variant",
          "launcher", "tile", "split", "generic", "text")
GROUP = re.compile(r'^et(\d+):(-|e\d+) 1:(-|[kK]\d+) 6:(-|[kK]\d+) 7:(-|[kK]\d+) 9:(-|[kK]\d+) 10:(-|[kK]\d+)$')
ETS, EKS = [0, 1, 2, 6, 10, 21], [1, 6, 7, 9, 10]
F32_EDGE = {0: 0, 1: 1, 2: 1, 6: 6, 10: 10, 21: 0}  # edge-tile mode -> what it is for an f32 call


def eligible(r):
    """everything but the tile: f32, planned on the generic kernel without having been forced there, no transposed operand, no VNNI C,
    k >= 64 a multiple of 8 but not of 64, a batch element, 16-byte pieces of every operand"""
    return (r["dt"] == "f32" and r["variant"] == 8 and r["forced"] != 8 and not r["a_trans"] and not r["b_trans"] and not r["vnni_c"] and
            r["k"] >= 64 and r["k"] % 8 == 0 and r["k"] % 64 != 0 and r["br"] >= 1 and r["n"] % 4 == 0 and
            all(r[x] % 4 == 0 and r[x] < 1 << 22 for x in ("lda", "ldb", "ldc")) and r["ab16"] and r["c16"] and ("B" not in r["ep"] or r["d16"]))


def edge_k_rule(r, et, ek):
    """the decision of an eligible call, None = stays where it is: the forced tile (edge_k, else a forcing edge-tile mode), else the
    edge tiles' rule; a tile that does not divide m and n only with the f32 edge tiles on"""
    if not eligible(r):
        return None
    fe = F32_EDGE[et]
    v = edge_rule(r["m"], r["n"], ek if ek != 1 else fe if fe in TILE else 1, r["cus"])
    if v is None:
        return None
    bm, bn = TILE[v]
    ragged = r["m"] % bm != 0 or r["n"] % bn != 0
    if ragged and not fe:
        return None
    return ("K" if ragged else "k") + str(v)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_edge_k")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_edge_k", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_edge_k")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    """one row per line, edge-tile mode and edge_k mode: base = the decision under the edge-tile mode alone ("-" / "e<variant>"),
    dec = the one with edge_k on top (None for "-"). A decision the driver had to print in full does not match and fails here"""
    out = []
    for l in table.splitlines():
        parts = l.split(" | ")
        m = HEAD.match(parts[0])
        assert m, "unreadable line: " + l
        base = dict(zip(FIELDS, m.groups()))
        for k in FIELDS:
            if k not in ("dt", "ep", "launcher", "text"):
                base[k] = int(base[k])
        assert len(parts) == 1 + len(ETS), l
        for et, g in zip(ETS, parts[1:]):
            gm = GROUP.match(g)
            assert gm and int(gm.group(1)) == et, "a decision that is neither the edge-tile mode's nor a ragged-k launch: " + l
            for ek, dec in zip(EKS, gm.groups()[2:]):
                out.append(dict(base, et=et, ek=ek, base=gm.group(2), dec=None if dec == "-" else dec, line=l))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's ragged-k choices differ from tests/golden/gemm_plan_edge_k.txt:\n" + diff)


def test_every_decision_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        want = edge_k_rule(r, r["et"], r["ek"])
        assert r["dec"] == want, (r["et"], r["ek"], want, r["line"])
        if r["dec"]:
            chosen += 1
            bm, bn = TILE[int(r["dec"][1:])]
            assert r["m"] >= bm and r["n"] >= bn and r["launcher"] == "generic", r["line"]
        if r["k"] % 64 != 0 or r["k"] < 64:
            assert r["base"] == "-", ("an edge-tile mode alone leaves a ragged k where it is", r["line"])
    assert chosen > 500


def test_case_list_covers_what_the_rule_depends_on(rows):
    assert {r["cus"] for r in rows} == {256, 64} and {r["et"] for r in rows} == set(ETS) and {r["ek"] for r in rows} == set(EKS)
    shapes = {(r["m"], r["n"]) for r in rows if r["k"] == 72 and r["br"] == 1}
    for bm, bn in TILE.values():
        assert {(bm + dm, bn + dn) for dm in (-1, 0, 1, bm) for dn in (-4, 0, 4, 2, bn)} <= shapes
    assert {r["k"] for r in rows} >= {32, 56, 64, 72, 96, 100, 127, 128, 200, 784, 1000} and {r["br"] for r in rows} >= {0, 1, 3}
    assert any(r["ldc"] % 4 for r in rows) and any(r["lda"] % 4 for r in rows) and any(r["ldb"] % 4 for r in rows)
    assert any(not r["ab16"] for r in rows) and any(not r["c16"] for r in rows)
    assert {("B" in r["ep"], r["d16"]) for r in rows} == {(False, 1), (False, 0), (True, 1), (True, 0)}
    assert any(r["forced"] == 8 for r in rows) and any(r["dt"] == "bf16" for r in rows)
    assert any(r["a_trans"] for r in rows) and any(r["b_trans"] for r in rows) and any(r["vnni_c"] for r in rows)
    mode1 = {r["dec"] for r in rows if r["ek"] == 1 and r["dec"]}
    assert mode1 >= {"k6", "k7", "k9", "k10"} and {d[0] for d in mode1} == {"k", "K"}, mode1
    # ragged m / n: nothing with the edge tiles off (or on for bf16 only), a launch with them on
    rag = [r for r in rows if (r["m"], r["n"], r["k"], r["br"], r["ep"], r["forced"]) == (1000, 1000, 1000, 1, "b", -1) and r["ek"] == 1]
    assert {r["et"]: r["dec"] for r in rag if r["cus"] == 256} == {0: None, 21: None, 1: "K6", 2: "K6", 6: "K6", 10: "K10"}
    # k = 96 under the edge-tile modes alone stays untouched
    assert all(r["base"] == "-" for r in rows if r["k"] == 96)


def test_the_named_shapes_get_the_expected_tile(rows):
    def pick(m, n, k, et=0, cus=256):
        got = {r["dec"] for r in rows if (r["m"], r["n"], r["k"], r["br"], r["cus"], r["et"], r["ek"], r["ep"], r["forced"]) == (m, n, k, 1, cus, et, 1, "b", -1)
               and r["dt"] == "f32" and r["ldc"] == n and r["ldb"] == n and r["lda"] == k and r["ab16"] and r["c16"] and not (r["a_trans"] or r["b_trans"] or r["vnni_c"])}
        assert len(got) == 1, (m, n, k, got)
        return got.pop()
    assert pick(1024, 1024, 1000) == "k6"     # 256 tiles of 64x64: one round
    assert pick(512, 1024, 784) == "k7"       # 256 tiles of 64x32
    assert pick(256, 1024, 200) == "k9"       # 256 tiles of 32x32 before 64 of 64x64
    assert pick(128, 1024, 72) == "k9"
    assert pick(2048, 1024, 1000) == "k10"    # 512 tiles of 64x64 in two rounds against 256 of 128x64 in one
    assert pick(1000, 1000, 1000) is None and pick(1000, 1000, 1000, et=1) == "K6"
    assert pick(1024, 1024, 1000, cus=64) == "k10"


def test_ragged_k_instances_exist_and_use_no_scratch():
    """brgemm_f32_lw_kedge<WM, WN, WK, NL, NSLOT, NLB>: 64x64 + K2, 64x32 + K4, 32x32 + K4 and 128x64 with the loader waves of the edge
    launch of each tile"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    src = os.path.join(CSRC, "brgemm_f32_lw.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "k.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch), (len(names), len(scratch))
    kedge = {n: s for n, s in zip(names, scratch) if n.startswith("_ZN3tpp19brgemm_f32_lw_kedgeI")}
    for args in ((2, 2, 2, 2, 4, 2), (2, 1, 4, 2, 4, 1), (1, 1, 4, 1, 4, 1), (4, 2, 1, 2, 3, 2)):
        want = "_ZN3tpp19brgemm_f32_lw_kedgeI" + "".join("Li%dE" % a for a in args) + "EE"
        assert any(n.startswith(want) for n in kedge), (want, sorted(kedge))
    assert len(kedge) == 4 and not {n: s for n, s in kedge.items() if s}, kedge
