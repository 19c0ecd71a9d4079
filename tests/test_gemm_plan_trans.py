"""CPU check of the planner's rule for gemms that read an operand transposed (tpp-mlir_amd/csrc/gemm_plan.cpp trans_launch; the siblings
the runtime makes of a gemm behind a folded transpose, xsmm_hip_set_fold_transpose modes 1 and 2): tests/gemm_plan_trans/driver.cpp steps
B-transposed and A-transposed siblings of both modes - 32x32x64, 64x48x64, 40x34x36, 36x48x40, 64x64x4, 34x32x32, k = 30, source leading
dimensions 512 / 52 / 50, strides and leading dimensions off the 4-float grid and around 2^24, bf16 and VNNI operands - through
plan_gemm_group and plan_gemm_call with every pointer aligned and not. tests/golden/gemm_plan_trans.txt is the reviewed record; whatever
the table says, every line must also satisfy the rule's invariants (below). And, compile-only: the new brgemm_grouped instances exist in
the gfx950 code object and use no scratch."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_trans.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

LINE = re.compile(r'^(A|B|AB) mode([12]) (\d+)x(\d+)x(\d+) lda(\d+) ldb(\d+) sa(\d+) sb(\d+) (f32|bf16) vnni([01]) vec([01]) : '
                  r'(\S+) (\S+) "([^"]*)" \| (\S+) (\S+) "([^"]*)"$')
FIELDS = ("form", "mode", "m", "n", "k", "lda", "ldb", "sa", "sb", "dt", "vnni", "vec", "launcher", "inst", "text", "c_launcher", "c_inst", "c_text")
NAMES = {"f32": "brgemm_grouped<f32>, B read transposed", "f32_bt_vec": "brgemm_grouped<f32,v4>, B read transposed",
         "f32_at_vec": "brgemm_grouped<f32,v4>, A read transposed", "f32_at": "brgemm_grouped<f32>, A read transposed"}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan_trans")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan_trans", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan_trans")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


@pytest.fixture(scope="module")
def rows(table):
    out = []
    for l in table.splitlines():
        m = LINE.match(l)
        assert m, "unreadable line: " + l
        r = dict(zip(FIELDS, m.groups()), line=l)
        for k in ("mode", "m", "n", "k", "lda", "ldb", "sa", "sb", "vnni", "vec"):
            r[k] = int(r[k])
        out.append(r)
    return out


def test_planner_reproduces_the_golden_table(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's choices for transposed operands differ from tests/golden/gemm_plan_trans.txt:\n" + diff)


def test_case_list_covers_what_the_rule_depends_on(rows):
    ok = [r for r in rows if r["dt"] == "f32" and not r["vnni"] and r["form"] != "AB"]
    assert {(r["m"], r["n"], r["k"]) for r in ok} >= {(32, 32, 64), (64, 48, 64), (40, 34, 36), (36, 48, 40), (64, 64, 4), (34, 32, 32), (32, 32, 30)}
    for form, ld in (("B", "ldb"), ("A", "lda")):
        mine = [r for r in ok if r["form"] == form]
        assert {r[ld] for r in mine} >= {512, 52, 50}
        assert {(r["mode"], r["vec"]) for r in mine} == {(1, 0), (1, 1), (2, 0), (2, 1)}
        assert {r["inst"] for r in mine if r["mode"] == 2} == ({"f32", "f32_bt_vec"} if form == "B" else {"f32_at", "f32_at_vec"})
    assert any(r["lda"] >= 1 << 24 for r in ok) and any(r["ldb"] >= 1 << 24 for r in ok)
    assert any(r["sa"] % 4 for r in ok) and any(r["sb"] % 4 for r in ok)


def test_every_line_keeps_the_rule(rows):
    for r in rows:
        l = r["line"]
        if r["dt"] != "f32" or r["vnni"] or r["form"] == "AB":  # bf16, a VNNI B operand, both operands: no kernel
            assert (r["launcher"], r["c_launcher"]) == ("invalid", "invalid"), l
            continue
        assert (r["launcher"], r["c_launcher"]) == ("generic", "generic"), l
        assert r["inst"] == r["c_inst"], l  # a single invoke runs on the instance its group of one alignment class would
        assert r["c_text"] == "", l
        vec16 = (r["mode"] == 2 and r["vec"] and r["k"] % 4 == 0 and all(r[x] % 4 == 0 for x in ("lda", "ldb", "sa", "sb")) and
                 r["lda"] < 1 << 24 and r["ldb"] < 1 << 24 and (r["form"] == "B" or (r["m"] % 4 == 0 and r["n"] % 4 == 0)))
        if r["form"] == "B":
            if r["mode"] == 1:
                assert r["inst"] == "f32", "a mode-1 sibling left the element path: " + l
            assert r["inst"] == ("f32_bt_vec" if vec16 else "f32"), l
        else:
            assert r["inst"] == ("f32_at_vec" if vec16 else "f32_at"), l
        assert r["text"] == NAMES[r["inst"]], l


def test_new_grouped_instances_exist_and_use_no_scratch():
    """brgemm_grouped<float, false, VEC, 2, FORM>: FORM 1 (B transposed) with 16-byte loads, FORM 2 (A transposed) with and without"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    src = os.path.join(CSRC, "brgemm_f32.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", os.path.join(tmp, "k.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch), (len(names), len(scratch))
    grouped = {n: s for n, s in zip(names, scratch) if n.startswith("_ZN3tpp14brgemm_groupedI")}
    for vec, form in ((1, 1), (1, 2), (0, 2)):
        want = "_ZN3tpp14brgemm_groupedIfLb0ELb%dELi2ELi%dEEE" % (vec, form)
        assert any(n.startswith(want) for n in grouped), (want, sorted(grouped))
    assert len(grouped) >= 9, sorted(grouped)
    bad = {n: s for n, s in grouped.items() if s != 0}
    assert not bad, "spilling instances of the generic kernel: %s" % bad
