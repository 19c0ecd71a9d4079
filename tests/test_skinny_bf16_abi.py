"""CPU-side checks of the skinny-batch bf16 switch (include/tpp_xsmm_abi.h xsmm_hip_set_skinny_bf16 / xsmm_hip_skinny_bf16_stats): the header
declares both symbols, the library exports them, tpp-mlir_amd/runtime.py wraps them, the setter takes 0, 1, 16, 32 and 64 only and returns
the previous mode, the five counters start at zero, TPP_HIP_SKINNY_BF16 is read when the library is loaded, the neighbouring switches keep
their values - and the code object of brgemm_bf16_skinny.hip holds exactly the sixteen instances of its table, without scratch or spills
(compile only, no GPU)."""
import importlib
import os
import re
import subprocess
import sys

import pytest

import skinny_codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("tpp-mlir_amd")
rtmod = importlib.import_module("tpp-mlir_amd.runtime")
SYMBOLS = ("xsmm_hip_set_skinny_bf16", "xsmm_hip_skinny_bf16_stats")
MODES = (0, 1, 16, 32, 64)
NEIGHBOURS = ("set_dma256_edge", "set_dma256_images", "set_edge_tiles", "set_edge_k", "set_edge_k_bf16", "set_edge_k8_bf16", "set_tail_split")


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
    assert hasattr(rt, "set_skinny_bf16") and hasattr(rt, "skinny_bf16_stats")


def test_the_setter_takes_its_five_modes_only_and_returns_the_previous_mode(rt):
    first = rt.set_skinny_bf16(0)
    assert first in MODES
    try:
        prev = 0
        for mode in MODES[1:] + (64, 0):
            assert rt.set_skinny_bf16(mode) == prev, mode
            prev = mode
        for bad in (-1, 2, 8, 15, 17, 24, 48, 128, 1001):
            assert rt.set_skinny_bf16(1) == 0
            assert rt.set_skinny_bf16(bad) == -1, bad
            assert rt.set_skinny_bf16(0) == 1, "a refused value changed the mode"
        stats = rt.skinny_bf16_stats()
        assert len(stats) == 5 and all(isinstance(v, int) for v in stats) and stats[0] >= 0
    finally:
        rt.set_skinny_bf16(first)


def test_the_neighbouring_switches_keep_their_values(rt):
    before = {}
    for name in NEIGHBOURS:
        before[name] = getattr(rt, name)(0)
        getattr(rt, name)(before[name])
    first = rt.set_skinny_bf16(64)
    try:
        for name in NEIGHBOURS:
            assert getattr(rt, name)(before[name]) == before[name], name
        rt.set_dma256_edge(2)
        assert rt.set_skinny_bf16(1) == 64 and rt.set_dma256_edge(before["set_dma256_edge"]) == 2
    finally:
        rt.set_skinny_bf16(first)


def child(env_value):
    env = {k: v for k, v in os.environ.items() if k != "TPP_HIP_SKINNY_BF16"}
    if env_value is not None:
        env["TPP_HIP_SKINNY_BF16"] = env_value
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(rt.skinny_bf16_stats(), rt.set_skinny_bf16(0))" % ROOT)
    return subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]


def test_the_environment_variable_is_read_in_a_child_process():
    """processes of their own: no launch has been counted; without the variable the mode is 0, a value the setter refuses is 0 too"""
    assert child(None) == "(0, 0, 0, 0, 0) 0"
    assert child("1") == "(0, 0, 0, 0, 0) 1"
    assert child("32") == "(0, 0, 0, 0, 0) 32"
    assert child("2") == "(0, 0, 0, 0, 0) 0"


def test_the_code_object_holds_exactly_the_instances_of_the_table_without_scratch():
    k = skinny_codeobj.resource_usage()
    assert sorted(k) == sorted(skinny_codeobj.KERNELS.values()) and len(k) == 16, sorted(k)
    for (img, bn, mb), name in skinny_codeobj.KERNELS.items():
        r = k[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgprs"] + r["agprs"] <= 256, (name, r)  # eight waves a workgroup: two per SIMD
        assert r["static_lds"] == skinny_codeobj.partial_lds_bytes(bn, mb) <= 64 * 1024, (name, r)
    with open(os.path.join(ROOT, "tpp-mlir_amd", "csrc", "brgemm_bf16_skinny.h")) as f:
        assert "constexpr int SKN_WMAX = %d;" % skinny_codeobj.WMAX in f.read()
