"""The narrow-output f32 kernel (include/tpp_xsmm_abi.h xsmm_hip_set_narrow_f32) without a GPU: the switch's plumbing and the six instances
of the gfx950 code object. The maps of brgemm_f32_narrow.h are checked where they run: tests/test_narrow_f32_gpu.py."""
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
ACCEPTED, WORDS = (0, 1, 16, 32, 64), 4
INSTANCES = [(bm, nb) for bm in (16, 32, 64) for nb in (16, 32)]


@pytest.fixture(scope="module")
def rt():
    pkg.build()
    return pkg.get_runtime()


def test_header_export_wrapper_setter_and_counters(rt):
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        header = f.read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    for s, sig in (("xsmm_hip_set_narrow_f32", (ctypes.c_int, [ctypes.c_int])), ("xsmm_hip_narrow_f32_stats", (None, [ctypes.POINTER(ctypes.c_int64)]))):
        assert re.search(r"TPP_XSMM_EXPORT\s+\w+\s+%s\s*\(" % s, header) and " T %s\n" % s in exported and hasattr(rt.lib, s) and rtmod._SIGNATURES[s] == sig, s
    assert type(rt).set_narrow_f32.__doc__ and type(rt).narrow_f32_stats.__doc__
    assert re.findall(r"xsmm_hip_narrow_f32_stats\s*\(\s*int64_t\s+out\[(\d+)\]", header) == [str(WORDS)]
    prev, last = rt.set_narrow_f32(0), 0
    for v in list(range(-2, 70)) + [128, 1016, 2 ** 31 - 1, -2 ** 31, prev]:
        assert rt.set_narrow_f32(v) == (last if v in ACCEPTED else -1), v
        last = v if v in ACCEPTED else last
    buf = (ctypes.c_int64 * (WORDS + 1))(*([-7] * (WORDS + 1)))
    rt.lib.xsmm_hip_narrow_f32_stats(buf)
    assert buf[WORDS] == -7 and tuple(buf[:WORDS]) == rt.narrow_f32_stats() and len(rt.narrow_f32_stats()) == WORDS


@pytest.mark.parametrize("text,want", [(None, 0), ("-1", 0), ("65", 0), ("1", 1), ("64", 64)])
def test_the_environment_variable_in_a_child_process(rt, text, want):
    env = {k: v for k, v in os.environ.items() if k != "TPP_HIP_NARROW_F32"}
    env.update({} if text is None else {"TPP_HIP_NARROW_F32": text})
    code = ("import importlib, json, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(json.dumps([list(rt.narrow_f32_stats()), rt.set_narrow_f32(0), rt.set_narrow_bf16(0)]))" % ROOT)
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]
    assert json.loads(out) == [[0] * WORDS, want, 0]


def test_the_six_instances_fit_the_budget():
    usage = resource_usage(os.path.join(CSRC, "brgemm_f32_narrow.hip"))
    assert sorted(usage) == sorted("_ZN3tpp17brgemm_f32_narrowILi%dELi%dEEEvNS_8GemmArgsE" % i for i in INSTANCES)
    for name, u in usage.items():
        bm, nb = (int(x) for x in re.findall(r"Li(\d+)E", name))
        assert u["scratch"] == 0 and u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0 and u["vgprs"] + u["agprs"] <= 256, (name, u)
        assert u["static_lds"] == 7 * (bm // 16) * (nb // 16) * 1024, (name, u)
