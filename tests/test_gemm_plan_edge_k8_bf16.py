"""CPU check of the planner's half-step bf16 ragged-k rule (tpp-mlir_amd/csrc/gemm_plan.cpp plan_gemm_call, xsmm_hip_set_edge_k8_bf16):
tests/gemm_plan_edge_k8_bf16/driver.cpp steps whole-layer bf16 calls - m, n in {128, 256, 1000, 1024, 4096}, k in {72, 200, 1000, 784, 1024},
the three B images, one and three batch elements - through plan_gemm and plan_gemm_call at 256 and 304 compute units under edge_k8_bf16 0,
1 and 21 crossed with edge-tile modes 0, 2 and 22 and the older ragged-k switch 0 and 1. One line per m, n, k and image, equal answers merged;
tests/golden/gemm_plan_edge_k8_bf16.txt is the reviewed record. Whatever the table says: with the new switch 0 every decision is the one of
an environment that never names the field; k = 784 and k = 1024 never report a half step; a k % 16 == 8 never reports the older switch's
", ragged k" launch; and every decision satisfies the rule as restated here from its issue (kedge8_rule).
And, compile-only: the twelve half-step instances exist in the gfx950 code object, use no scratch and at most 256 VGPRs."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_edge_k8_bf16.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

SHAPE = re.compile(r'^(\d+)x(\d+)x(\d+) vf(\d)$')
OFF = re.compile(r'^v(\d+) (\S+) t(\d+) s(\d+) b(\d+) "([^"]*)"$')
GROUP = re.compile(r'^((?:\d+/\d,)*\d+/\d)=(-|[ekK]\d+) (-|[hH]\d+) (-|[hH]\d+) (-|[hH]\d+)$')
SIZES, KS_ALL = (128, 256, 1000, 1024, 4096), (72, 200, 1000, 784, 1024)
ETS, OLD, NEW = [0, 2, 22], [0, 1], [0, 1, 21]
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]  # 32x64 + K2, 64x64, 64x128, 128x128: variant 20 + t (VNNI-2), 24 + t (flat), 28 + t (VNNI-4)
IMAGE_BASE = {2: 20, 0: 24, 4: 28}
# the fitted model of the divisible shapes (profiles/r06_bf16_sweep.txt): a round of workgroups of tile t costs A[t] + B[t] x chunks us
BLW_A, BLW_B = (3.56, 3.75, 4.66, 6.06), (0.098, 0.135, 0.204, 0.236)
V_GENERIC, V_SMALL32 = 8, 19


def k8_ok(k):
    return k >= 64 and k % 8 == 0 and k % 16 != 0


def kedge8_rule(m, n, k, br, et, mode, cus, variant=V_GENERIC):
    """the tile index a call takes whose operands are eligible (bf16, no VNNI C, nothing forced, planned on `variant` = the generic or the
    32x32 K-split kernel, n % 8 == 0, a batch element, the alignment facts), None = it stays where it is - restated from the issue.
    k >= 64, k % 8 == 0, k % 16 != 0. Candidates: the tiles that fit and, unless a bf16 edge-tile mode (2, 20 .. 23) is on, divide m and
    n. A forcing value of this switch names the tile, else a forcing edge-tile mode does - if it is a candidate; else the gate - a call on
    the K-split kernel whose 32x32 tiles fit one round of the CUs with br * k < 1024 stays - and then the cheapest candidate by
    rounds(ceil-divided tiles, CUs) x (A + B x br x ceil(k / 64)), ties to the larger tile"""
    if mode == 0 or not k8_ok(k) or n % 8 or br < 1 or variant not in (V_GENERIC, V_SMALL32):
        return None
    edge_on = et == 2 or 20 <= et <= 23
    cand = [t for t, (bm, bn) in enumerate(TILE) if m >= bm and n >= bn and (edge_on or (m % bm == 0 and n % bn == 0))]
    forced = mode - 20 if 20 <= mode <= 23 else et - 20 if 20 <= et <= 23 else None
    if forced is not None:
        return forced if forced in cand else None
    assert mode == 1
    if variant == V_SMALL32 and (m // 32) * (n // 32) <= cus and br * k < 1024:
        return None
    chunks = br * -(-k // 64)
    cost = lambda t: -(-((-(-m // TILE[t][0])) * (-(-n // TILE[t][1]))) // cus) * (BLW_A[t] + BLW_B[t] * chunks)  # noqa: E731
    return min(cand, key=lambda t: (cost(t), -t)) if cand else None


def want_decision(r):
    t = kedge8_rule(r["m"], r["n"], r["k"], r["br"], r["et"], r["new"], r["cus"], r["variant"])
    if t is None:
        return None
    bm, bn = TILE[t]
    return ("H" if r["m"] % bm or r["n"] % bn else "h") + str(IMAGE_BASE[r["vf"]] + t)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_edge_k8_bf16")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_edge_k8_bf16", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_edge_k8_bf16")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    """one row per call (m, n, k, image, batch count, CU count), edge-tile mode, old-switch mode and new-switch mode: base = the decision without the new field ("-" / "e<variant>"
    / "k<variant>" / "K<variant>"), dec = the one with edge_k8_bf16 on top (None for "-"). A decision the driver had to print in full does
    not match and fails here"""
    out = []
    for l in table.splitlines():
        parts = l.split(" | ")
        m = SHAPE.match(parts[0])
        assert m and len(parts) > 1, "unreadable line: " + l
        shape = dict(zip(("m", "n", "k", "vf"), (int(x) for x in m.groups())))
        for part in parts[1:]:
            keys, _, body = part.partition(" : ")
            fields = body.split(" ; ")
            om = OFF.match(fields[0])
            assert om, "unreadable decision: " + l
            off = dict(zip(("variant", "launcher", "tile", "split", "b_kind", "text"), om.groups()))
            for f in ("variant", "tile", "split", "b_kind"):
                off[f] = int(off[f])
            for key in keys.split(","):
                br, cus = (int(x) for x in re.match(r"^br(\d+)c(\d+)$", key).groups())
                for g in fields[1:]:
                    gm = GROUP.match(g)
                    assert gm, "a decision that is neither the older switches' nor a half-step launch: " + l
                    for eo in gm.group(1).split(","):
                        et, old = (int(x) for x in eo.split("/"))
                        for new, dec in zip(NEW, gm.groups()[2:]):
                            out.append(dict(shape, **off, br=br, cus=cus, et=et, old=old, new=new, base=gm.group(2), dec=None if dec == "-" else dec,
                                            line="%s br%d cus%d" % (l, br, cus)))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's half-step ragged-k choices differ from tests/golden/gemm_plan_edge_k8_bf16.txt:\n" + diff)


def test_the_table_has_every_case(rows):
    keys = {(r["m"], r["n"], r["k"], r["vf"], r["br"], r["cus"], r["et"], r["old"], r["new"]) for r in rows}
    assert keys == {(m, n, k, vf, br, cus, et, old, new) for m in SIZES for n in SIZES for k in KS_ALL for vf in (2, 0, 4) for br in (1, 3)
                    for cus in (256, 304) for et in ETS for old in OLD for new in NEW}
    assert len(rows) == len(keys) == 1500 * 18


def test_switch_off_is_the_row_without_the_field(rows):
    assert all(r["dec"] is None for r in rows if r["new"] == 0)


def test_the_two_switches_partition_the_lengths(rows):
    for r in rows:
        if r["k"] in (784, 1024):
            assert r["dec"] is None and "half step" not in r["text"], ("k % 16 == 0 is never the new switch's", r["line"])
        if r["k"] % 16 == 8:
            assert r["base"][0] not in "kK" and ", ragged k" not in r["text"], ("k % 16 == 8 is never the old switch's", r["line"])
            assert r["base"] == "-", ("the older switches leave such a call where it is", r["line"])
    # the old switch goes on taking its own lengths with the new one on
    assert any(r["k"] == 784 and r["old"] == 1 and r["new"] == 1 and r["base"][0] in "kK" for r in rows)
    assert not any(r["k"] == 784 and r["old"] == 0 and r["base"][0] in "kK" for r in rows)


def test_every_decision_keeps_the_rule(rows):
    chosen = 0
    for r in rows:
        want = want_decision(r)
        assert r["dec"] == want, (r["et"], r["old"], r["new"], want, r["line"])
        if r["dec"]:
            chosen += 1
            bm, bn = TILE[int(r["dec"][1:]) & 3]
            assert r["m"] >= bm and r["n"] >= bn and r["launcher"] in ("generic", "bf16_small32"), r["line"]
            assert r["dec"][0] == "h" or r["et"] in (2, 22), ("a tile that does not divide m and n needs the edge tiles", r["line"])
            assert k8_ok(r["k"])
    assert chosen > 3000
    # the old switch's mode changes nothing about the new one's decision
    by = {}
    for r in rows:
        by.setdefault((r["line"], r["et"], r["new"]), set()).add(r["dec"])
    assert all(len(v) == 1 for v in by.values())


def test_the_named_shapes_get_the_expected_tile(rows):
    def pick(m, n, k, et=0, cus=256, vf=2, new=1, br=1):
        got = {r["dec"] for r in rows if (r["m"], r["n"], r["k"], r["br"], r["cus"], r["et"], r["new"], r["vf"]) == (m, n, k, br, cus, et, new, vf)}
        assert len(got) == 1, (m, n, k, got)
        return got.pop()
    # 1024 x 1024 x 1000 (16 chunks): 256 tiles of 64x64 in one round (5.9 us by the model) against 128 of 64x128 (7.9) and 64 of 128x128 (9.8)
    assert pick(1024, 1024, 1000) == "h21" and pick(1024, 1024, 1000, vf=0) == "h25" and pick(1024, 1024, 1000, vf=4) == "h29"
    assert pick(4096, 1024, 1000) == "h23" and pick(4096, 1024, 1000, cus=304) == "h23"
    # no K-split kernel takes a k that is no multiple of 16: these calls are the generic kernel's with every image, the gate never holds
    assert pick(256, 1024, 200) == "h20" and pick(256, 1024, 200, vf=0) == "h24" and pick(128, 1024, 72) == "h20"
    assert pick(1000, 1000, 1000) is None and pick(1000, 1000, 1000, et=2) == "H21" and pick(1000, 1000, 1000, et=22) == "H22"
    assert pick(1000, 1000, 1000, new=21) is None and pick(1000, 1000, 1000, et=22, new=21) == "H21"
    assert pick(1024, 1024, 1000, new=21) == "h21" and pick(1024, 1024, 1000, et=22) == "h22"
    assert pick(1024, 1024, 784) is None and pick(1024, 1024, 1024) is None
    assert {r["variant"] for r in rows if r["k"] % 16 == 8} == {V_GENERIC}


def test_half_step_instances_exist_and_use_no_scratch():
    """brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, 1, false, FLATB, 6>: the four tiles with the loader waves and ring of the plain
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
    half = {n: (s, v) for n, s, v in zip(names, scratch, vgprs) if n.endswith("Li6EEEvNS_9ChainArgsE")}
    tiles = ((1, 2, 2, 1, 1, 8, 1, 2, 1), (2, 2, 1, 1, 1, 8, 1, 1, 1), (2, 2, 1, 1, 2, 6, 1, 2, 1), (2, 2, 1, 2, 2, 4, 1, 1, 1))
    for args in tiles:
        for image in (0, 2, 4):
            want = "_ZN3tpp14brgemm_bf16_lwI" + "".join("Li%dE" % a for a in args) + "Lb0ELi%dELi6EEEvNS_9ChainArgsE" % image
            assert want in half, (want, sorted(half))
    assert len(half) == 12, sorted(half)
    assert not {n: x for n, x in half.items() if x[0] or x[1] > 256}, half
