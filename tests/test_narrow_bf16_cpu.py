"""The narrow-output bf16 kernel (include/tpp_xsmm_abi.h xsmm_hip_set_narrow_bf16) without a GPU: the switch's plumbing, the maps of
brgemm_bf16_narrow.h walked as the kernel walks them (tests/narrow_bf16/driver.cpp), and the eighteen instances of the gfx950 code object."""
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
ACCEPTED, WORDS = (0, 1, 16, 32, 64), 5
INSTANCES = [(img, bm, nb) for img in (0, 2, 4) for bm in (16, 32, 64) for nb in (16, 32)]


@pytest.fixture(scope="module")
def rt():
    pkg.build()
    return pkg.get_runtime()


def test_header_export_wrapper_setter_and_counters(rt):
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        header = f.read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    for s, sig in (("xsmm_hip_set_narrow_bf16", (ctypes.c_int, [ctypes.c_int])), ("xsmm_hip_narrow_bf16_stats", (None, [ctypes.POINTER(ctypes.c_int64)]))):
        assert re.search(r"TPP_XSMM_EXPORT\s+\w+\s+%s\s*\(" % s, header) and " T %s\n" % s in exported and hasattr(rt.lib, s) and rtmod._SIGNATURES[s] == sig, s
    assert type(rt).set_narrow_bf16.__doc__ and type(rt).narrow_bf16_stats.__doc__
    assert re.findall(r"xsmm_hip_narrow_bf16_stats\s*\(\s*int64_t\s+out\[(\d+)\]", header) == [str(WORDS)]
    prev, last = rt.set_narrow_bf16(0), 0
    for v in list(range(-2, 70)) + [128, 1016, 2 ** 31 - 1, -2 ** 31, prev]:
        assert rt.set_narrow_bf16(v) == (last if v in ACCEPTED else -1), v
        last = v if v in ACCEPTED else last
    buf = (ctypes.c_int64 * (WORDS + 1))(*([-7] * (WORDS + 1)))
    rt.lib.xsmm_hip_narrow_bf16_stats(buf)
    assert buf[WORDS] == -7 and tuple(buf[:WORDS]) == rt.narrow_bf16_stats() and len(rt.narrow_bf16_stats()) == WORDS


@pytest.mark.parametrize("text,want", [(None, 0), ("-1", 0), ("65", 0), ("1", 1), ("64", 64)])
def test_the_environment_variable_in_a_child_process(rt, text, want):
    env = {k: v for k, v in os.environ.items() if k != "TPP_HIP_NARROW_BF16"}
    env.update({} if text is None else {"TPP_HIP_NARROW_BF16": text})
    code = ("import importlib, json, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(json.dumps([list(rt.narrow_bf16_stats()), rt.set_narrow_bf16(0), rt.set_skinny_bf16(0)]))" % ROOT)
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]
    assert json.loads(out) == [[0] * WORDS, want, 0]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("narrow_bf16") / "driver")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++14", "-O1", "-I" + CSRC, os.path.join(ROOT, "tests", "narrow_bf16", "driver.cpp"), "-o", exe])
    return lambda *a: subprocess.run([exe] + [str(x) for x in a], capture_output=True, text=True, check=True, timeout=300).stdout.strip()


@pytest.mark.parametrize("img,bm,nb", INSTANCES)
def test_the_maps_walked_for_one_shape_per_instance(driver, img, bm, nb):
    # clamped rows in the last block, a partly used column set, a ragged last step, three batch elements: every element once, nothing outside
    m, n, k, br = 2 * bm + 7, (10 if nb == 16 else 31), 72, 3
    want = "waves 8 a_once %d of %d b_once %d of %d c_once %d of %d bad 0" % ((br * m * k,) * 2 + (br * k * n,) * 2 + (m * n,) * 2)
    assert driver(img, bm, m, n, k, br) == want
    assert driver(img, bm, 32, nb - 15, 8, 1).startswith("waves 1 a_once 256 of 256 ") and driver(img, bm, 32, nb - 1, 8, 1).endswith(" bad 0")


def test_the_eighteen_instances_fit_the_budget():
    usage = resource_usage(os.path.join(CSRC, "brgemm_bf16_narrow.hip"))
    assert sorted(usage) == sorted("_ZN3tpp18brgemm_bf16_narrowILi%dELi%dELi%dEEEvNS_8GemmArgsE" % i for i in INSTANCES)
    for name, u in usage.items():
        img, bm, nb = (int(x) for x in re.findall(r"Li(\d+)E", name))
        assert u["scratch"] == 0 and u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0 and u["vgprs"] + u["agprs"] <= 256, (name, u)
        assert u["static_lds"] == 7 * (bm // 16) * (nb // 16) * 4 * 64 * 4 <= 64 << 10, (name, u)
