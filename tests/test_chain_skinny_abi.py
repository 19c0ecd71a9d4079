"""CPU-side checks of the switch for skinny-batch layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_skinny / xsmm_hip_chain_skinny_stats):
the header declares both symbols, the library exports them, tpp-mlir_amd/runtime.py wraps them, the setter takes 0, 1, 16 / 32 / 64 and
1000 * G + BN with 1 <= G <= 512 only and returns the previous mode, the four counters start at zero, TPP_HIP_CHAIN_SKINNY is read when the
library is loaded, the seven other chain switches and the two skinny switches keep their values - and the code object of
brgemm_bf16_skinny_chain.hip holds exactly the sixteen instances of the unsplit kernel's table, without scratch or spills, within 256
registers and with the unsplit kernel's LDS (compile only, no GPU)."""
import importlib
import os
import re
import subprocess
import sys

import pytest

import chain_skinny_codeobj
import skinny_codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("tpp-mlir_amd")
rtmod = importlib.import_module("tpp-mlir_amd.runtime")
SYMBOLS = ("xsmm_hip_set_chain_skinny", "xsmm_hip_chain_skinny_stats")
NEIGHBOURS = ("set_chain_edge", "set_chain_rounds", "set_chain_ragged", "set_chain_widths", "set_chain_width_rounds", "set_chain_widths_ragged", "set_chain_dma256",
              "set_skinny_bf16", "set_skinny_split")
GOOD = [1, 16, 32, 64, 1016, 2016, 3032, 512064, 1, 0]
BAD = [-1, 2, 8, 17, 48, 65, 128, 1000, 1001, 1008, 2017, 513016, 600016, 1000 * 0x10000 + 16]


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
    assert hasattr(rt, "set_chain_skinny") and hasattr(rt, "chain_skinny_stats")


def test_the_setter_takes_its_modes_only_and_returns_the_previous_mode(rt):
    first = rt.set_chain_skinny(0)
    try:
        prev = 0
        for mode in GOOD:
            assert rt.set_chain_skinny(mode) == prev, mode
            prev = mode
        for bad in BAD:
            assert rt.set_chain_skinny(1) == 0
            assert rt.set_chain_skinny(bad) == -1, bad
            assert rt.set_chain_skinny(0) == 1, "a refused value changed the mode"
        stats = rt.chain_skinny_stats()
        assert len(stats) == 4 and all(isinstance(v, int) for v in stats) and stats[0] >= 0
    finally:
        rt.set_chain_skinny(first)


def test_the_other_chain_switches_and_the_skinny_switches_keep_their_values(rt):
    before = {}
    for name in NEIGHBOURS:
        before[name] = getattr(rt, name)(0)
        getattr(rt, name)(before[name])
    first = rt.set_chain_skinny(2016)
    try:
        for name in NEIGHBOURS:
            assert getattr(rt, name)(before[name]) == before[name], name
        rt.set_skinny_bf16(32), rt.set_skinny_split(3), rt.set_chain_dma256(2)
        assert rt.set_chain_skinny(1) == 2016
        assert rt.set_skinny_bf16(before["set_skinny_bf16"]) == 32 and rt.set_skinny_split(before["set_skinny_split"]) == 3
        assert rt.set_chain_dma256(before["set_chain_dma256"]) == 2
    finally:
        rt.set_chain_skinny(first)


def child(env_value):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}
    if env_value is not None:
        env["TPP_HIP_CHAIN_SKINNY"] = env_value
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(rt.chain_skinny_stats(), rt.set_chain_skinny(0), rt.set_skinny_bf16(0), rt.set_skinny_split(0), rt.set_chain_dma256(0))" % ROOT)
    return subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]


def test_the_environment_variable_is_read_in_a_child_process():
    """processes of their own: no launch has been counted; without the variable the mode is 0, a value the setter refuses is 0 too; no
    other switch reads this variable"""
    assert child(None) == "(0, 0, 0, 0) 0 0 0 0"
    assert child("1") == "(0, 0, 0, 0) 1 0 0 0"
    assert child("64") == "(0, 0, 0, 0) 64 0 0 0"
    assert child("3032") == "(0, 0, 0, 0) 3032 0 0 0"
    assert child("2") == "(0, 0, 0, 0) 0 0 0 0"
    assert child("600016") == "(0, 0, 0, 0) 0 0 0 0"
    assert child("-1") == "(0, 0, 0, 0) 0 0 0 0"


def test_the_code_object_holds_exactly_the_sixteen_instances_without_scratch():
    k = chain_skinny_codeobj.resource_usage()
    assert sorted(k) == sorted(chain_skinny_codeobj.KERNELS.values()) and len(k) == 16, sorted(k)
    for (img, bn, mb), name in chain_skinny_codeobj.KERNELS.items():
        r = k[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgprs"] + r["agprs"] <= 256, (name, r)  # eight waves a workgroup: two per SIMD
        assert r["static_lds"] == skinny_codeobj.partial_lds_bytes(bn, mb) <= 64 * 1024, (name, r)
