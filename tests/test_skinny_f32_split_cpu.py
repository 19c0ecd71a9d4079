"""The K split across workgroups of the skinny-batch f32 kernel (include/tpp_xsmm_abi.h xsmm_hip_set_skinny_f32_split) without a GPU: the
maps of brgemm_f32_skinny_split.h walked by brute force, the planner's cells with the real gemm_plan.cpp at 256 CUs
(tests/skinny_f32_split/driver.cpp), the switch's plumbing, and the six instances of the gfx950 code object."""
import importlib
import os
import re
import subprocess
import sys

import pytest

from skinny_codeobj import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
pkg = importlib.import_module("tpp-mlir_amd")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("skinny_f32_split")
    objs = []
    for src in (os.path.join(CSRC, "gemm_plan.cpp"), os.path.join(ROOT, "tests", "skinny_f32_split", "driver.cpp")):
        objs.append(str(d / (os.path.basename(src) + ".o")))
        subprocess.check_call([build.hipcc()] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", objs[-1]])
    subprocess.check_call([build.hipcc(), "--offload-arch=" + build.ARCH] + objs + ["-o", str(d / "driver")])
    return lambda a: subprocess.run([str(d / "driver"), a], capture_output=True, text=True, check=True, timeout=300).stdout


def test_every_step_in_one_part_and_wave_the_scratch_disjoint_and_the_three_limits(driver):
    want = ["deal steps %d P %d parts %d once %d bad 0" % (s, p, min(s, p), s) for s in (1, 2, 3, 9, 32, 63) for p in (2, 3, 4, 16)]
    want += ["scratch bn %d mb %d floats %d once %d bad 0" % (bn, mb, 15 * mb * bn, 15 * mb * bn) for bn in (16, 64) for mb in (16, 32)]
    assert driver("maps").splitlines() == want + ["fits 1 0 1 0 1 0 0"]


# call: the cells of (skinny_f32, skinny_f32_split) = (16, 0) (16, 4) (32, 16) (0, 3) (1, 1) (1, 0); "-" = the launch with both switches off.
# Mode 1 of the split, as fitted to profiles/skinny_f32_split_ab.txt (gemm_plan.cpp skinny_f32_split_parts): P = 4, else 2, where a
# workgroup of the unsplit launch streams at least 256 KiB of B (4 BN br k) and blocks * P <= CUs; else the plain launch
U, S = "brgemm_f32_skinny<%dx%d>/%d/1", "brgemm_f32_skinny_split<%dx%d>/%d/%d"


def cells(mb, rule_bn, rule_p, steps=64):
    rule = "-" if not rule_bn else (S % (mb, rule_bn, rule_bn, rule_p) if rule_p > 1 else U % (mb, rule_bn, rule_bn))
    return [U % (mb, 16, 16), S % (mb, 16, 16, min(4, steps)), S % (mb, 32, 32, min(16, steps)), "-", rule, "-" if not rule_bn else U % (mb, rule_bn, rule_bn)]


PLAN = {"m1 n1024 K1024": cells(16, 16, 1), "m1 n1024 K4096": cells(16, 16, 4), "m1 n4096 K4096": cells(16, 32, 2),
        "m16 n1024 K1024": cells(16, 16, 1), "m16 n1024 K4096": cells(16, 16, 4), "m16 n4096 K4096": cells(16, 32, 2),
        "m31 n1024 K1024": cells(32, 16, 1), "m31 n1024 K4096": cells(32, 16, 4), "m31 n4096 K4096": cells(32, 0, 1),
        "m8 n64 k36 br1": cells(16, 0, 1, steps=3), "m8 n64 k16 br1": [U % (16, 16, 16), U % (16, 16, 16), U % (16, 32, 32), "-", "-", "-"], "m32": ["-"] * 6}


def test_the_planner_cells_split_off_forced_skinny_off_and_mode_1(driver):
    assert {l.split(" : ")[0][5:]: l.split(" : ")[1].split() for l in driver("plan").splitlines()} == PLAN


def test_setter_environment_and_counter_plumbing():
    pkg.build()
    rt = pkg.get_runtime()
    prev, last = rt.set_skinny_f32_split(0), 0
    for v in list(range(0, 17)) + [17, -1, prev]:
        ok = 0 <= v <= 16
        assert rt.set_skinny_f32_split(v) == (last if ok else -1), v
        last = v if ok else last
    assert len(rt.skinny_f32_split_stats()) == 3
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        assert re.findall(r"TPP_XSMM_EXPORT\s+void\s+xsmm_hip_skinny_f32_split_stats\s*\(\s*int64_t\s+out\[(\d+)\]", f.read()) == ["3"]
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(list(rt.skinny_f32_split_stats()), rt.set_skinny_f32_split(0), rt.set_skinny_f32(0), rt.set_skinny_split(0))" % ROOT)
    for text, want in (("16", 16), ("17", 0), ("-1", 0)):
        env = dict({k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}, TPP_HIP_SKINNY_F32_SPLIT=text)
        assert subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1] == "[0, 0, 0] %d 0 0" % want


def test_the_six_instances_are_in_the_code_object_with_no_scratch_and_the_unsplit_lds():
    usage = resource_usage(os.path.join(CSRC, "brgemm_f32_skinny_split.hip"))
    assert sorted(usage) == sorted("_ZN3tpp23brgemm_f32_skinny_splitILi%dELi%dEEEvNS_8GemmArgsE" % (bn, mb) for bn in (16, 32, 64) for mb in (16, 32))
    for name, u in usage.items():
        bn, mb = (int(x) for x in re.findall(r"Li(\d+)E", name))
        assert u["scratch"] == 0 and u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0 and u["vgprs"] + u["agprs"] <= 256, (name, u)
        assert u["static_lds"] == 7 * (mb // 16) * (bn // 16) * 4 * 64 * 4 <= 56 << 10, (name, u)
