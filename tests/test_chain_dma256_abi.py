"""CPU-side checks of the switch for layer chains on the 256x256 bf16 tile (include/tpp_xsmm_abi.h xsmm_hip_set_chain_dma256 /
xsmm_hip_chain_dma256_stats): the header declares both symbols, the library exports them, tpp-mlir_amd/runtime.py wraps them, the setter takes
0, 1, 2 and 1000 + G only and returns the previous mode, the counters start at zero, TPP_HIP_CHAIN_DMA256 is read when the library is
loaded, the neighbouring switches are unmoved - and the code object of brgemm_bf16_dma256_chain.hip holds exactly the three instances,
without scratch (compile only, no GPU)."""
import importlib
import os
import re
import subprocess
import sys

import pytest

import chain_dma256_codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("tpp-mlir_amd")
rtmod = importlib.import_module("tpp-mlir_amd.runtime")
SYMBOLS = ("xsmm_hip_set_chain_dma256", "xsmm_hip_chain_dma256_stats")


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


def test_the_setter_takes_0_1_2_and_forced_groups_and_returns_the_previous_mode(rt):
    first = rt.set_chain_dma256(0)
    assert first == 0 or first in (1, 2) or first > 1000
    try:
        assert rt.set_chain_dma256(1) == 0 and rt.set_chain_dma256(2) == 1 and rt.set_chain_dma256(1001) == 2 and rt.set_chain_dma256(1064) == 1001
        assert rt.set_chain_dma256(1000 + 0x10000) == 1064 and rt.set_chain_dma256(0) == 1000 + 0x10000
        for bad in (-1, 3, 18, 1000, 1000 + 0x10000 + 1):
            assert rt.set_chain_dma256(1) == 0
            assert rt.set_chain_dma256(bad) == -1, bad
            assert rt.set_chain_dma256(0) == 1, "a refused value changed the mode"
        stats = rt.chain_dma256_stats()
        assert len(stats) == 4 and all(isinstance(v, int) for v in stats) and stats[0] >= 0
        # a switch of its own: the neighbours keep their values
        rt.set_chain_dma256(2)
        assert rt.set_chain_rounds(0) == 0 and rt.set_dma256_edge(0) == 0 and rt.set_dma256_images(0) == 0
        assert rt.set_chain_rounds(1) == 0 and rt.set_dma256_edge(1) == 0 and rt.set_dma256_images(1) == 0
        assert rt.set_chain_dma256(0) == 2
        assert rt.set_chain_rounds(0) == 1 and rt.set_dma256_edge(0) == 1 and rt.set_dma256_images(0) == 1
    finally:
        rt.set_chain_dma256(first)


def child(env_value):
    env = {k: v for k, v in os.environ.items() if k != "TPP_HIP_CHAIN_DMA256"}
    if env_value is not None:
        env["TPP_HIP_CHAIN_DMA256"] = env_value
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(rt.chain_dma256_stats(), rt.set_chain_dma256(0), rt.set_chain_rounds(0), rt.set_dma256_images(0))" % ROOT)
    return subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]


def test_the_environment_variable_is_read_in_a_child_process():
    """processes of their own: no launch has been counted; without the variable the mode is 0, a value the setter refuses is 0 too; the
    variable sets no other switch"""
    assert child(None) == "(0, 0, 0, 0) 0 0 0"
    assert child("2") == "(0, 0, 0, 0) 2 0 0"
    assert child("1") == "(0, 0, 0, 0) 1 0 0"
    assert child("1016") == "(0, 0, 0, 0) 1016 0 0"
    assert child("3") == "(0, 0, 0, 0) 0 0 0"
    assert child("1000") == "(0, 0, 0, 0) 0 0 0"


def test_the_code_object_holds_the_three_chain_kernels_without_scratch():
    k = chain_dma256_codeobj.resource_usage()
    assert sorted(k) == sorted(chain_dma256_codeobj.KERNELS.values()), sorted(k)
    for name, r in k.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgprs"] + r["agprs"] <= 512, (name, r)
        assert r["static_lds"] == 0, (name, r)  # the ring is dynamic LDS: the launcher's figure below
    assert chain_dma256_codeobj.launcher_lds_bytes() == 128 * 1024
