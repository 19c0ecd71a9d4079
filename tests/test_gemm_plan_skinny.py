"""CPU regression of the planner under the skinny-batch bf16 switch (tpp-mlir_amd/csrc/gemm_plan.cpp plan_gemm_call,
xsmm_hip_set_skinny_bf16): tests/gemm_plan_skinny/driver.cpp steps whole-layer calls - m in {1, 8, 16, 17, 31, 32, 33} x n in {8, 16, 24, 64,
72, 1000, 1024, 4096} x k in {8, 32, 40, 64, 1000, 1024} at 1 and 16 batch elements x the three B images, and f32, a VNNI C, forced kernels, an
empty batch, the epilogues, each misalignment, wide, off-grid and short leading dimensions, n % 8 and k % 8 - through plan_gemm and
plan_gemm_call under modes 0, 1, 16, 32 and 64 at 64, 256 and 304 compute units, strict mode off and on, alone and with every other switch
on. tests/golden/gemm_plan_skinny.txt is the reviewed table; the rule is restated here from the header's contract text."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_skinny.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

DESC = re.compile(r"^(v2|v4|flat|vc|f32) (\d+)x(\d+)x(\d+)(?: ld(\d+),(\d+),(\d+))? e(\S+) f(-?\d+) : (\d+) (\S+)( gf)?( vf)?$")
CALL = re.compile(r"^ c br(\d+)(?: a(\d+)/(\d+)/(\d+))? : (.*) \| 1: (\S+) (\S+) (\S+) \| 16: (\S+) \| 32: (\S+) \| 64: (\S+)$")
VFAC = {"v2": 2, "v4": 4, "flat": 1}
MS, NS, KS = (1, 8, 16, 17, 31, 32, 33), (8, 16, 24, 64, 72, 1000, 1024, 4096), (8, 32, 40, 64, 1000, 1024)
V_GENERIC = 8


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_skinny")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_skinny", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_skinny")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=300).stdout


@pytest.fixture(scope="module")
def rows(table):
    out, desc = [], None
    for l in table.splitlines():
        m = DESC.match(l)
        if m:
            g = m.groups()
            k = int(g[3])
            desc = dict(form=g[0], m=int(g[1]), n=int(g[2]), k=k, ld=tuple(int(x) for x in g[4:7]) if g[4] else (16 * k, int(g[2]), int(g[2])),
                        lattice=not g[4], ep=g[7], forced=int(g[8]), variant=int(g[9]), gf=bool(g[11]), vf=bool(g[12]), desc_line=l)
            continue
        c = CALL.match(l)
        assert c and desc, "unreadable line (a '!' marks a violated invariant): " + l
        g = c.groups()
        out.append(dict(desc, br=int(g[0]), ab=int(g[1] or 16), c=int(g[2] or 16), d=int(g[3] or 16), m0=g[4], rule=g[5:8], forced_bn={16: g[8], 32: g[9], 64: g[10]},
                        line=desc["desc_line"] + " /" + l))
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's choices under xsmm_hip_set_skinny_bf16 differ from tests/golden/gemm_plan_skinny.txt:\n" + diff)


def test_no_line_marks_a_violated_invariant(table):
    """the driver's own checks: mode 0 is an environment that never names the field, strict mode gives the same answer, a forcing mode does
    not read the compute units, no other switch changes this one, a taken launch is the skinny launcher with its text"""
    assert "!" not in table, [l for l in table.splitlines() if "!" in l][:5]


def test_the_table_has_the_whole_lattice(rows):
    for form in VFAC:
        got = {(r["m"], r["n"], r["k"], r["br"]) for r in rows if r["form"] == form and r["lattice"] and r["forced"] == -1 and r["ep"] == "bBr" and r["ab"] == 16}
        assert {(m, n, k, br) for m in MS for n in NS for k in KS for br in (1, 16)} <= got
    assert {r["form"] for r in rows} == {"v2", "v4", "flat", "vc", "f32"}
    assert any(r["gf"] for r in rows) and any(r["br"] == 0 for r in rows) and any(r["ep"] == "-" for r in rows)
    assert {(r["ab"], r["c"], r["d"]) for r in rows} == {(16, 16, 16), (8, 16, 16), (16, 8, 16), (16, 4, 16), (16, 16, 4), (16, 16, 8)}


def eligible(r):
    """restated from the contract text of include/tpp_xsmm_abi.h"""
    if r["form"] not in VFAC or r["gf"] or r["vf"] or r["variant"] != V_GENERIC:
        return False
    m, n, k = r["m"], r["n"], r["k"]
    if not (1 <= m <= 31 and n % 8 == 0 and k >= 8 and k % 8 == 0 and r["br"] >= 1):
        return False
    lda, ldb, ldc = r["ld"]
    if lda < k or ldb < n or ldc < n or lda % 8 or ldb % 8 or ldc % 8:
        return False
    return r["ab"] >= 16 and r["c"] >= 16 and ("B" not in r["ep"] or r["d"] >= 8)


def instance(form, bn):
    return not (form == "flat" and bn == 16)


def rule_bn(r):
    """mode 1: the gate (m >= 17 on the generic kernel's 16-byte path - a VNNI B, k % 32 == 0), else by the bytes of B"""
    if r["form"] != "flat" and r["k"] % 32 == 0 and r["m"] > 16:
        return 0
    smallest, line = (32 if r["form"] == "flat" else 16), 64 // VFAC[r["form"]]
    bn = line if 2 * r["br"] * r["k"] * r["n"] >= 16 << 20 else smallest
    while bn > smallest and r["n"] < bn:
        bn //= 2
    return bn if r["n"] >= bn else 0


def cell(r, bn):
    return "S%dx%d" % (16 if r["m"] <= 16 else 32, bn) if bn else "-"


def test_every_row_keeps_the_rule(rows):
    taken = {1: 0, 16: 0, 32: 0, 64: 0}
    for r in rows:
        assert "skinny" not in r["m0"], r["line"]
        ok = eligible(r)
        for bn in (16, 32, 64):
            want = cell(r, bn if ok and instance(r["form"], bn) and r["n"] >= bn else 0)
            assert r["forced_bn"][bn] == want, (bn, r["line"])
            taken[bn] += want != "-"
        want = cell(r, rule_bn(r) if ok else 0)
        assert r["rule"] == (want,) * 3, r["line"]  # the measured rule does not read the compute units
        taken[1] += want != "-"
    assert all(v > 300 for v in taken.values()), taken


def test_what_is_never_taken(rows):
    for r in rows:
        if r["form"] in ("f32", "vc") or r["m"] >= 32 or r["gf"] or r["vf"] or r["br"] == 0 or r["n"] == 8:
            assert r["rule"] == ("-",) * 3 and set(r["forced_bn"].values()) == {"-"}, r["line"]
    # a forced BN with n < BN stays
    for r in rows:
        if r["form"] == "v2" and r["lattice"] and r["m"] == 8 and r["k"] == 64 and r["br"] == 1 and r["ep"] == "bBr" and r["forced"] == -1 and r["ab"] == r["c"] == r["d"] == 16:
            if r["n"] in (16, 24):
                assert (r["forced_bn"][16], r["forced_bn"][32], r["forced_bn"][64]) == ("S16x16", "-", "-"), r["line"]
            if r["n"] == 72:
                assert (r["forced_bn"][16], r["forced_bn"][32], r["forced_bn"][64]) == ("S16x16", "S16x32", "S16x64"), r["line"]


def test_the_measured_rows(rows):
    """profiles/skinny_bf16_ab.txt: the rows that decided mode 1 (VNNI-2 unless named), as K = br x k"""
    def pick(form, m, n, k, br):
        got = {r["rule"][1] for r in rows if (r["form"], r["m"], r["n"], r["k"], r["br"]) == (form, m, n, k, br) and r["lattice"] and r["forced"] == -1
               and r["ep"] == "bBr" and r["ab"] == r["c"] == r["d"] == 16}
        assert len(got) == 1, (form, m, n, k, br, got)
        return got.pop()
    for m in (1, 8, 16):
        assert pick("v2", m, 4096, 1024, 16) == "S16x32"       # B 256 MiB: the BN of one line per row piece
        assert pick("v2", m, 1024, 64, 16) == "S16x16"         # 1024 x 1024: B 2 MiB
        assert pick("v2", m, 4096, 64, 16) == "S16x16"         # 4096 x 1024: B 8 MiB
        assert pick("v2", m, 1000, 1000, 1) == "S16x16"        # the generic kernel's element path
        assert pick("v4", m, 4096, 1024, 16) == "S16x16" and pick("flat", m, 4096, 1024, 16) == "S16x64"
        assert pick("flat", m, 1024, 64, 16) == "S16x32"
    for m in (17, 31):
        assert pick("v2", m, 1024, 64, 16) == "-" and pick("v2", m, 4096, 1024, 16) == "-" and pick("v4", m, 4096, 1024, 16) == "-"  # the gate
        assert pick("v2", m, 1000, 1000, 1) == "S32x16" and pick("v2", m, 1024, 40, 1) == "S32x16" and pick("flat", m, 1024, 64, 16) == "S32x32"
