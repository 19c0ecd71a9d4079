"""CPU check of the GEMM kernel planner (tpp-mlir_amd/csrc/gemm_plan.cpp): tests/gemm_plan/driver.cpp steps a fixed case list -
named shapes, the reference's benchmark layers as whole-layer calls and tile invokes, operand forms, alignments and lane-offset
limits, forced variants, forced split counts, strict mode, work-list lengths, quads - through plan_gemm, plan_gemm_call,
plan_gemm_group and the quads model, one line per decision. The planner is compiled with hipcc and the library's own flags, so
the floating-point near-ties are decided as in the shipped code. The expected table, tests/golden/gemm_plan.txt, is what the
launchers chose before the planner was split out of them; a change of a rule or a coefficient is a reviewed change of that table."""
import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan.txt")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402


@pytest.fixture(scope="module")
def plan_table(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_plan")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (os.path.join(ROOT, "tests", "gemm_plan", "driver.cpp"), "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "plan")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout


def test_planner_reproduces_the_golden_table(plan_table):
    with open(GOLDEN) as f:
        want = f.read()
    if plan_table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), plan_table.splitlines(True), "golden", "planner"))[:80])
        pytest.fail("the planner's choices differ from tests/golden/gemm_plan.txt:\n" + diff)


def test_table_covers_every_forced_variant_and_launcher(plan_table):
    lines = plan_table.splitlines()
    forced = {int(m.group(1)) for m in (re.search(r" f(-?\d+) : ", l) for l in lines) if m}
    assert set(range(32)) <= forced
    launchers = {l.split(" : ")[1].split()[0].split("<")[0] for l in lines if l.split()[1] in ("c", "g", "q")}
    assert launchers >= {"f32_fast", "f32_lw", "f32_lw16", "f32_lw_grouped", "f32_x6", "bf16_fast", "bf16_small32", "bf16_grouped64",
                         "bf16_lw", "bf16_lw_grouped", "bf16_lw_quads", "generic", "invalid"}
