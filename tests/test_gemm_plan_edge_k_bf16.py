"""CPU check of the planner's bf16 ragged-k rule (tpp-mlir_amd/csrc/gemm_plan.cpp plan_gemm_call / choose_bf16_kedge_tile,
xsmm_hip_set_edge_k_bf16): tests/gemm_plan_edge_k_bf16/driver.cpp steps whole-layer calls - m = BM - 1, BM, BM + 1 and n = BN - 8, BN, BN + 8,
BN + 4 around each of the four tiles, k = 48, 64, 72, 80, 96, 128, 784, no / one / three batch elements, each leading dimension off its
grid, each alignment bit off, a bias row with and without its 8 bytes, the three B images, forced kernels, a VNNI C, f32 controls and the
whole layers of the A/B - through plan_gemm and plan_gemm_call at 256 and 64 compute units under edge_k_bf16 0, 1, 20 .. 23 crossed with
edge-tile modes 0, 2 and 21. One line per call and CU count; tests/golden/gemm_plan_edge_k_bf16.txt is the reviewed record. Whatever the
table says, every decision must also satisfy the rule as restated here from its issue, and a mode that does not apply must leave the
decision of the same edge-tile mode untouched, field by field.
And, compile-only: the twelve ragged-k instances exist in the gfx950 code object, use no scratch and at most 256 VGPRs."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_edge_k_bf16.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

HEAD = re.compile(r'^(\d+)x(\d+)x(\d+) br(\d+) (f32|bf16) vf(\d) vc([01]) e(\S*) lda(\d+) ldb(\d+) ldc(\d+) al([01])([01])([01]) f(-?\d+) cus(\d+) : '
                  r'v(\d+) vfd([01]) (\S+) t(\d+) s(\d+) b(\d+) g(\d+) "([^"]*)"$')
FIELDS = ("m", "n", "k", "br", "dt", "vf", "vnni_c", "ep", "lda", "ldb", "ldc", "ab16", "c16", "d8", "forced", "cus", "variant", "variant_forced",
          "launcher", "tile", "split", "b_kind", "generic", "text")
GROUP = re.compile(r'^et(\d+):(-|e\d+|f\d+) 1:(-|[kK]\d+) 20:(-|[kK]\d+) 21:(-|[kK]\d+) 22:(-|[kK]\d+) 23:(-|[kK]\d+)$')
ETS, EKS = [0, 2, 21], [1, 20, 21, 22, 23]
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]  # 32x64 + K2, 64x64, 64x128, 128x128: variant 20 + t (VNNI-2), 24 + t (flat), 28 + t (VNNI-4)
IMAGE_BASE = {2: 20, 0: 24, 4: 28}
# the fitted model of the divisible shapes (profiles/r06_bf16_sweep.txt): a round of workgroups of tile t costs A[t] + B[t] x chunks us
BLW_A, BLW_B = (3.56, 3.75, 4.66, 6.06), (0.098, 0.135, 0.204, 0.236)


def k_ok(k):
    return k >= 64 and k % 16 == 0 and k % 64 != 0


def eligible(r):
    """everything but the tile: bf16 without a VNNI C, planned on the generic or the 32x32 K-split kernel without having been forced there,
    k >= 64 a multiple of 16 but not of 64, a batch element, n in 16-byte pieces, the image's leading dimensions and lane offsets, A / B /
    C on 16 bytes and a bias row on 8"""
    ldb_ok = {2: r["ldb"] % 4 == 0 and r["ldb"] < 1 << 21, 0: r["ldb"] % 8 == 0 and r["ldb"] < 1 << 21, 4: r["ldb"] % 2 == 0 and r["ldb"] < 1 << 20}
    stride_a, stride_b = r["k"], r["k"] * r["ldb"]  # the driver's layers
    return (r["dt"] == "bf16" and not r["vnni_c"] and r["forced"] != 8 and not r["variant_forced"] and r["variant"] in (8, 19) and k_ok(r["k"]) and
            r["br"] >= 1 and r["n"] % 8 == 0 and all(r[x] % 8 == 0 and r[x] < 1 << 22 for x in ("lda", "ldc")) and stride_a % 8 == 0 and
            stride_b % 8 == 0 and ldb_ok[r["vf"]] and r["ab16"] and r["c16"] and ("B" not in r["ep"] or r["d8"]))


def kedge_rule(m, n, k, br, et, ek, cus):
    """the tile index an eligible call takes, None = it stays where it is - restated from the issue. Candidates: the tiles that fit and,
    unless a bf16 edge-tile mode (2, 20 .. 23) is on, divide m and n. A forcing edge_k_bf16 value's tile, else a forcing edge-tile mode's,
    if it is a candidate; else the cheapest by rounds(ceil-divided tiles, CUs) x (A + B x br x ceil(k / 64)), ties to the larger tile"""
    edge_on = et == 2 or 20 <= et <= 23
    cand = [t for t, (bm, bn) in enumerate(TILE) if m >= bm and n >= bn and (edge_on or (m % bm == 0 and n % bn == 0))]
    forced = ek - 20 if 20 <= ek <= 23 else et - 20 if 20 <= et <= 23 else None
    if forced is not None:
        return forced if forced in cand else None
    assert ek == 1
    chunks = br * -(-k // 64)
    cost = lambda t: -(-((-(-m // TILE[t][0])) * (-(-n // TILE[t][1]))) // cus) * (BLW_A[t] + BLW_B[t] * chunks)  # noqa: E731
    return min(cand, key=lambda t: (cost(t), -t)) if cand else None


def gated(r):
    """the rule's gate (measured: profiles/edge_k_bf16_ab.txt): with no tile forced, a call planned on the 32x32 K-split kernel whose 32x32
    tiles fit one round of the CUs and whose reduction is below 1024 stays there"""
    forced = 20 <= r["ek"] <= 23 or 20 <= r["et"] <= 23
    return not forced and r["variant"] == 19 and (r["m"] // 32) * (r["n"] // 32) <= r["cus"] and r["br"] * r["k"] < 1024


def want_decision(r):
    if not eligible(r) or gated(r):
        return None
    t = kedge_rule(r["m"], r["n"], r["k"], r["br"], r["et"], r["ek"], r["cus"])
    if t is None:
        return None
    bm, bn = TILE[t]
    return ("K" if r["m"] % bm or r["n"] % bn else "k") + str(IMAGE_BASE[r["vf"]] + t)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_edge_k_bf16")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_edge_k_bf16", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_edge_k_bf16")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    """one row per line, edge-tile mode and edge_k_bf16 mode: base = the decision under the edge-tile mode alone ("-" / "e<variant>" /
    "f<tile>" for an f32 control), dec = the one with edge_k_bf16 on top (None for "-"). A decision the driver had to print in full does
    not match and fails here"""
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
        pytest.fail("the planner's bf16 ragged-k choices differ from tests/golden/gemm_plan_edge_k_bf16.txt:\n" + diff)


def test_every_decision_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        want = want_decision(r)
        assert r["dec"] == want, (r["et"], r["ek"], want, r["line"])
        if r["dec"]:
            chosen += 1
            bm, bn = TILE[int(r["dec"][1:]) & 3]
            assert r["m"] >= bm and r["n"] >= bn and r["n"] % 8 == 0 and r["launcher"] in ("generic", "bf16_small32"), r["line"]
            assert r["dec"][0] == "k" or r["et"] in (2, 21), ("a tile that does not divide m and n needs the edge tiles", r["line"])
        if not k_ok(r["k"]) or r["dt"] != "bf16":
            assert r["dec"] is None, ("not this switch's call", r["line"])
        if r["k"] % 64 != 0 and r["dt"] == "bf16":
            assert r["base"] == "-", ("an edge-tile mode alone leaves a ragged k where it is", r["line"])
    assert chosen > 500


def test_case_list_covers_what_the_rule_depends_on(rows):
    bf = [r for r in rows if r["dt"] == "bf16"]
    assert {r["cus"] for r in rows} == {256, 64} and {r["et"] for r in rows} == set(ETS) and {r["ek"] for r in rows} == set(EKS)
    for k, br in ((80, 1), (784, 3)):
        shapes = {(r["m"], r["n"]) for r in bf if r["k"] == k and r["br"] == br and r["vf"] == 2}
        for bm, bn in TILE:
            assert {(bm + dm, bn + dn) for dm in (-1, 0, 1) for dn in (-8, 0, 8, 4)} <= shapes
    assert {r["k"] for r in bf} >= {48, 64, 72, 80, 96, 128, 784, 1000, 200} and {r["br"] for r in bf} >= {0, 1, 3}
    for vf, grid in ((2, 4), (0, 8), (4, 2)):
        assert any(r["vf"] == vf and r["ldb"] % grid for r in bf) and any(r["vf"] == vf and r["lda"] % 8 for r in bf)
        assert any(r["vf"] == vf and r["ldc"] % 8 for r in bf) and any(r["vf"] == vf and r["ldc"] != r["n"] and r["dec"] for r in bf)
    assert any(not r["ab16"] for r in bf) and any(not r["c16"] for r in bf)
    assert {("B" in r["ep"], r["d8"]) for r in bf} == {(False, 1), (False, 0), (True, 1), (True, 0)}
    assert any(r["forced"] == 8 for r in bf) and any(r["variant_forced"] for r in bf) and any(r["forced"] == 21 and not r["variant_forced"] for r in bf)
    assert any(r["vnni_c"] for r in bf) and any(r["dt"] == "f32" for r in rows)
    assert any(r["variant"] == 19 and r["dec"] for r in bf), "a call planned on the 32x32 K-split kernel is taken"
    mode1 = {r["dec"] for r in bf if r["ek"] == 1 and r["dec"]}
    assert mode1 >= {"k20", "k21", "k22", "k23", "k25", "k29"} and {d[0] for d in mode1} == {"k", "K"}, mode1
    # ragged m / n: nothing with the edge tiles off, a launch with them on
    rag = [r for r in bf if (r["m"], r["n"], r["k"], r["br"], r["vf"]) == (1000, 1000, 784, 1, 2) and r["ek"] == 1 and r["cus"] == 256]
    assert {r["et"]: r["dec"] for r in rag} == {0: None, 2: "K21", 21: "K21"}
    # an f32 call and k = 72, 1000, 48, 64, 128 stay untouched under every mode
    assert all(r["dec"] is None for r in rows if r["dt"] == "f32" or r["k"] in (48, 64, 72, 128, 200, 1000))


def test_the_named_shapes_get_the_expected_tile(rows):
    def pick(m, n, k, et=0, cus=256, vf=2, ek=1):
        got = {r["dec"] for r in rows if (r["m"], r["n"], r["k"], r["br"], r["cus"], r["et"], r["ek"], r["ep"], r["forced"], r["vf"], r["dt"]) ==
               (m, n, k, 1, cus, et, ek, "b", -1, vf, "bf16") and r["ldc"] == n and r["ab16"] and r["c16"]}
        assert len(got) == 1, (m, n, k, got)
        return got.pop()
    # 1024 x 1024 x 784 (13 chunks): 256 tiles of 64x64 in one round (5.5 us by the model) against 512 of 32x64 in two (9.7), 128 of
    # 64x128 (7.3) and 64 of 128x128 (9.1)
    assert pick(1024, 1024, 784) == "k21" and pick(1024, 1024, 784, vf=0) == "k25" and pick(1024, 1024, 784, vf=4) == "k29"
    assert pick(4096, 1024, 784) == "k23"     # 256 tiles of 128x128 in one round (9.1) against 512 of 64x128 in two (14.6)
    # 256 tiles of 32x32 on the K-split kernel, one round, K < 1024: gated (measured slower on the tiles); the flat image has no such kernel
    assert pick(256, 1024, 400) is None and pick(128, 1024, 80) is None
    assert pick(256, 1024, 400, vf=0) == "k24" and pick(128, 1024, 80, vf=0) == "k24"   # 128 tiles of 32x64 (4.2) before 64 of 64x64 (4.7)
    assert pick(256, 1024, 400, ek=20) == "k20" and pick(256, 1024, 400, cus=64) == "k21"  # a forced tile; four rounds of the K-split kernel
    assert pick(1000, 1000, 784) is None and pick(1000, 1000, 784, et=2) == "K21"
    assert pick(1024, 1024, 784, cus=64) == "k23"
    assert pick(1024, 1024, 784, ek=22) == "k22" and pick(1024, 1024, 784, et=21) == "k21" and pick(1024, 1024, 784, et=21, ek=23) == "k23"
    assert pick(1000, 1000, 784, ek=21) is None and pick(1000, 1000, 784, et=21, ek=20) == "K20"
    assert pick(1024, 1024, 832) is None      # whole chunks: the plain kernels' call


def test_ragged_k_instances_exist_and_use_no_scratch():
    """brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, 1, false, FLATB, 4>: the four tiles with the loader waves and ring of the plain
    launch of each, one chunk per barrier only, the three B images"""
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
    kedge = {n: (s, v) for n, s, v in zip(names, scratch, vgprs) if n.endswith("Li4EEEvNS_9ChainArgsE")}
    tiles = ((1, 2, 2, 1, 1, 8, 1, 2, 1), (2, 2, 1, 1, 1, 8, 1, 1, 1), (2, 2, 1, 1, 2, 6, 1, 2, 1), (2, 2, 1, 2, 2, 4, 1, 1, 1))
    for args in tiles:
        for image in (0, 2, 4):
            want = "_ZN3tpp14brgemm_bf16_lwI" + "".join("Li%dE" % a for a in args) + "Lb0ELi%dELi4EEEvNS_9ChainArgsE" % image
            assert want in kedge, (want, sorted(kedge))
    assert len(kedge) == 12, sorted(kedge)
    assert not {n: x for n, x in kedge.items() if x[0] or x[1] > 256}, kedge
