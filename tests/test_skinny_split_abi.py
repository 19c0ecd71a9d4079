"""CPU-side checks of the skinny split switch (include/tpp_xsmm_abi.h xsmm_hip_set_skinny_split / xsmm_hip_skinny_split_stats): the header
declares both symbols, the library exports them, tpp-mlir_amd/runtime.py wraps them, the setter takes 0 .. 16 only and returns the previous
mode, the three counters start at zero, TPP_HIP_SKINNY_SPLIT is read when the library is loaded, xsmm_hip_set_skinny_bf16 and its
neighbours keep their values - and the code object of brgemm_bf16_skinny_split.hip holds exactly the sixteen instances of the unsplit
kernel's table, without scratch or spills, within 256 registers and with the unsplit kernel's LDS (compile only, no GPU)."""
import importlib
import os
import re
import subprocess
import sys

import pytest

import skinny_codeobj
import skinny_split_codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("tpp-mlir_amd")
rtmod = importlib.import_module("tpp-mlir_amd.runtime")
SYMBOLS = ("xsmm_hip_set_skinny_split", "xsmm_hip_skinny_split_stats")
NEIGHBOURS = ("set_skinny_bf16", "set_dma256_edge", "set_dma256_images", "set_edge_tiles", "set_edge_k", "set_edge_k_bf16", "set_edge_k8_bf16", "set_tail_split")


@pytest.fixture(scope="module")
def rt():
    pkg.build()
    return pkg.get_runtime()


def test_the_header_declares_and_the_library_exports_both_symbols(rt):
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        declared = re.findall(r"TPP_XSMM_EXPORT\s+[\w\s\*]+?\b(\w+)\s*\(", f.read())
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in SYMBOLS:
        assert s in declared and s in exported and hasattr(rt.lib, s) and s in rtmod._SIGNATURES, s
    assert hasattr(rt, "set_skinny_split") and hasattr(rt, "skinny_split_stats")


def test_the_setter_takes_0_to_16_only_and_returns_the_previous_mode(rt):
    first = rt.set_skinny_split(0)
    assert 0 <= first <= 16
    try:
        prev = 0
        for mode in list(range(1, 17)) + [16, 0]:
            assert rt.set_skinny_split(mode) == prev, mode
            prev = mode
        for bad in (-1, 17, 1000):
            assert rt.set_skinny_split(1) == 0
            assert rt.set_skinny_split(bad) == -1, bad
            assert rt.set_skinny_split(0) == 1, "a refused value changed the mode"
        stats = rt.skinny_split_stats()
        assert len(stats) == 3 and all(isinstance(v, int) for v in stats) and stats[0] >= 0
    finally:
        rt.set_skinny_split(first)


def test_the_skinny_switch_and_its_neighbours_keep_their_values(rt):
    before = {}
    for name in NEIGHBOURS:
        before[name] = getattr(rt, name)(0)
        getattr(rt, name)(before[name])
    first = rt.set_skinny_split(16)
    try:
        for name in NEIGHBOURS:
            assert getattr(rt, name)(before[name]) == before[name], name
        rt.set_skinny_bf16(32)
        assert rt.set_skinny_split(1) == 16 and rt.set_skinny_bf16(before["set_skinny_bf16"]) == 32
    finally:
        rt.set_skinny_split(first)


def child(env_value):
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_SKINNY_SPLIT", "TPP_HIP_SKINNY_BF16")}
    if env_value is not None:
        env["TPP_HIP_SKINNY_SPLIT"] = env_value
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(rt.skinny_split_stats(), rt.set_skinny_split(0), rt.set_skinny_bf16(0))" % ROOT)
    return subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]


def test_the_environment_variable_is_read_in_a_child_process():
    """processes of their own: no launch has been counted; without the variable the mode is 0, a value the setter refuses is 0 too; the
    skinny switch does not read this variable"""
    assert child(None) == "(0, 0, 0) 0 0"
    assert child("1") == "(0, 0, 0) 1 0"
    assert child("16") == "(0, 0, 0) 16 0"
    assert child("17") == "(0, 0, 0) 0 0"
    assert child("-1") == "(0, 0, 0) 0 0"


def test_the_code_object_holds_exactly_the_sixteen_instances_without_scratch():
    k = skinny_split_codeobj.resource_usage()
    assert sorted(k) == sorted(skinny_split_codeobj.KERNELS.values()) and len(k) == 16, sorted(k)
    for (img, bn, mb), name in skinny_split_codeobj.KERNELS.items():
        r = k[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgprs"] + r["agprs"] <= 256, (name, r)  # eight waves a workgroup: two per SIMD
        assert r["static_lds"] == skinny_codeobj.partial_lds_bytes(bn, mb) <= 64 * 1024, (name, r)
