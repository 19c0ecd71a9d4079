"""The skinny-batch f32 kernel (include/tpp_xsmm_abi.h xsmm_hip_set_skinny_f32) without a GPU: the maps of brgemm_f32_skinny.h walked by
brute force and the planner's takes / stays under modes 0, 1, 16, 32, 64 (the real gemm_plan.cpp, tests/skinny_f32/driver.cpp), the
switch's plumbing as tests/test_mode_switches.py checks it for the other eighteen, and the six instances of the gfx950 code object."""
import ctypes
import importlib
import json
import os
import re
import subprocess
import sys

import pytest

from skinny_codeobj import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
pkg = importlib.import_module("tpp-mlir_amd")
rtmod = importlib.import_module("tpp-mlir_amd.runtime")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402
ACCEPTED, WORDS = (0, 1, 16, 32, 64), 4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("skinny_f32")
    objs = []
    for src in (os.path.join(CSRC, "gemm_plan.cpp"), os.path.join(ROOT, "tests", "skinny_f32", "driver.cpp")):
        objs.append(str(d / (os.path.basename(src) + ".o")))
        subprocess.check_call([build.hipcc()] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", objs[-1]])
    subprocess.check_call([build.hipcc(), "--offload-arch=" + build.ARCH] + objs + ["-o", str(d / "driver")])
    return lambda *a, **kw: subprocess.run([str(d / "driver")] + list(a), capture_output=True, text=True, check=True, timeout=300, **kw).stdout


def test_the_maps_by_brute_force(driver):
    want = []
    for bn in (16, 32, 64):
        want.append("slab bn %d once %d bad 0" % (bn, 16 * bn))
        want += ["store bn %d m %d n %d once %d bad 0" % (bn, m, n, m * n) for m in (1, 7, 16, 17, 31) for n in (bn, bn + 4, bn + 12, 200)]
    want += ["mask kmod %d steps %d kept_below %d bad 0" % (kmod, 3 if kmod else 2, 16 * (32 + kmod)) for kmod in (0, 4, 8, 12)]
    want += ["deal steps %d waves %d end %d bad 0" % (s, min(8, s), s) for s in (1, 3, 7, 8, 9, 43, 63)]
    assert driver("maps").splitlines() == want


# call: the cell under modes 0, 1, 16, 32, 64 - "-" = the launch of mode 0, else kernel text / BN. Mode 1 as fitted to
# profiles/skinny_f32_ab.txt (gemm_plan.cpp skinny_f32_bn): B of 4 MB .. 16 MiB on BN 16 (m >= 18: at most 64 column blocks), B >= 64 MiB on
# BN 32 for m <= 16, everything else gated
S16, S32 = "brgemm_f32_skinny<16x%d>/%d", "brgemm_f32_skinny<32x%d>/%d"
STAYS = ["m32", "n12", "n1022", "k6", "ldb1026", "unaligned C", "unaligned bias", "unaligned A", "bf16", "forced generic", "B transposed", "A transposed", "empty batch"]
PLAN = {"m8 n1024 k64 br16": ["-", S16 % (16, 16)] + [S16 % (bn, bn) for bn in (16, 32, 64)],
        "m31 n1000 k1000 beta1": ["-", S32 % (16, 16)] + [S32 % (bn, bn) for bn in (16, 32, 64)],
        "m17 n4096 k64 br64": ["-", "-"] + [S32 % (bn, bn) for bn in (16, 32, 64)],
        "m16 n4096 k64 br64": ["-", S16 % (32, 32)] + [S16 % (bn, bn) for bn in (16, 32, 64)],
        "m31 n4096 k64 br16": ["-", "-"] + [S32 % (bn, bn) for bn in (16, 32, 64)],
        "m1 n48 k4 strided": ["-", "-", S16 % (16, 16), S16 % (32, 32), "-"],
        "m16 n16 k16": ["-", "-", S16 % (16, 16), "-", "-"],
        **{what: ["-"] * 5 for what in STAYS}}


def test_the_planner_takes_and_stays_as_written_and_changes_no_golden_plan_with_m_at_least_32(driver):
    assert {l.split(" : ")[0][5:]: l.split(" : ")[1].split() for l in driver("plan").splitlines()} == PLAN
    pat = re.compile(r"^D\d+ (\w+) (\d+)x(\d+)x(\d+)(?: ld(\d+),(\d+),(\d+))?(?: s(\d+),(\d+))? e(\S+) f(-?\d+) :")
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan.txt")) as f:
        specs = [m.groups() for m in map(pat.match, f) if m and int(m.group(2)) >= 32]
    assert len(specs) > 50 and {"f32", "v2", "flat"} <= {s[0] for s in specs}
    out = driver("golden", input="".join(" ".join(x if x is not None else "-1" for x in s) + "\n" for s in specs))
    assert out.split() == ["golden", "descs", str(len(specs)), "differ", "0"]


@pytest.fixture(scope="module")
def rt():
    pkg.build()
    return pkg.get_runtime()


def test_header_export_wrapper_setter_and_counters(rt):
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        header = f.read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    for s, sig in (("xsmm_hip_set_skinny_f32", (ctypes.c_int, [ctypes.c_int])), ("xsmm_hip_skinny_f32_stats", (None, [ctypes.POINTER(ctypes.c_int64)]))):
        assert re.search(r"TPP_XSMM_EXPORT\s+\w+\s+%s\s*\(" % s, header) and " T %s\n" % s in exported and hasattr(rt.lib, s) and rtmod._SIGNATURES[s] == sig, s
    assert type(rt).set_skinny_f32.__doc__ and type(rt).skinny_f32_stats.__doc__
    assert re.findall(r"xsmm_hip_skinny_f32_stats\s*\(\s*int64_t\s+out\[(\d+)\]", header) == [str(WORDS)]
    prev, last = rt.set_skinny_f32(0), 0
    for v in list(range(-2, 70)) + [128, 1016, 2 ** 31 - 1, -2 ** 31, prev]:
        assert rt.set_skinny_f32(v) == (last if v in ACCEPTED else -1), v
        last = v if v in ACCEPTED else last
    buf = (ctypes.c_int64 * (WORDS + 1))(*([-7] * (WORDS + 1)))
    rt.lib.xsmm_hip_skinny_f32_stats(buf)
    assert buf[WORDS] == -7 and tuple(buf[:WORDS]) == rt.skinny_f32_stats() and len(rt.skinny_f32_stats()) == WORDS


@pytest.mark.parametrize("text,want", [(None, 0), ("-1", 0), ("65", 0), ("1", 1), ("64", 64)])
def test_the_environment_variable_in_a_child_process(rt, text, want):
    env = {k: v for k, v in os.environ.items() if k != "TPP_HIP_SKINNY_F32"}
    env.update({} if text is None else {"TPP_HIP_SKINNY_F32": text})
    code = ("import importlib, json, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(json.dumps([list(rt.skinny_f32_stats()), rt.set_skinny_f32(0), rt.set_skinny_bf16(0)]))" % ROOT)
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]
    assert json.loads(out) == [[0] * WORDS, want, 0]


def test_the_six_instances_fit_the_budget():
    usage = resource_usage(os.path.join(CSRC, "brgemm_f32_skinny.hip"))
    assert sorted(usage) == sorted("_ZN3tpp17brgemm_f32_skinnyILi%dELi%dEEEvNS_8GemmArgsE" % (bn, mb) for bn in (16, 32, 64) for mb in (16, 32))
    for name, u in usage.items():
        bn, mb = (int(x) for x in re.findall(r"Li(\d+)E", name))
        assert u["scratch"] == 0 and u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0 and u["vgprs"] + u["agprs"] <= 256, (name, u)
        assert u["static_lds"] == 7 * (mb // 16) * (bn // 16) * 4 * 64 * 4 <= 64 << 10, (name, u)
