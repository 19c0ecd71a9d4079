"""CPU-side checks of the mixed-width chain switch (include/tpp_xsmm_abi.h xsmm_hip_set_chain_widths / xsmm_hip_chain_widths_stats): the header
declares both symbols, the library exports them, tpp-mlir_amd/runtime.py wraps them, the setter takes 0 and 1 only and returns the previous
mode, the counters start at zero - and the weak stand-ins that let the host-only builds of runtime.cpp link are where the real definitions
override them."""
import importlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("tpp-mlir_amd")
SYMBOLS = ("xsmm_hip_set_chain_widths", "xsmm_hip_chain_widths_stats")


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
        assert s in declared and s in exported and hasattr(rt.lib, s), s


def test_the_setter_takes_0_and_1_only_and_returns_the_previous_mode(rt):
    first = rt.set_chain_widths(0)
    assert first in (0, 1)
    try:
        assert rt.set_chain_widths(1) == 0 and rt.set_chain_widths(1) == 1 and rt.set_chain_widths(0) == 1
        for bad in (-1, 2, 9, 20, 23, 1001):
            assert rt.set_chain_widths(bad) == -1, bad
            assert rt.set_chain_widths(0) == 0, "a refused value changed the mode"
        assert rt.set_chain_ragged(2) == -1 and rt.set_chain_edge(2) == -1, "the other chain switches still take 0 and 1 only"
        stats = rt.chain_widths_stats()
        assert len(stats) == 4 and all(isinstance(v, int) for v in stats) and stats[0] >= 0
    finally:
        rt.set_chain_widths(first)


def test_the_counters_start_at_zero_and_the_switch_is_off_by_default():
    """a process of its own: no launch has been counted, and without the environment variable the mode is 0"""
    env = {k: v for k, v in os.environ.items() if k != "TPP_HIP_CHAIN_WIDTHS"}
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(rt.chain_widths_stats(), rt.set_chain_widths(0))" % ROOT)
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120)
    assert out.strip().splitlines()[-1] == "(0, 0, 0, 0) 0", out


def test_the_real_planner_and_launcher_override_the_weak_stand_ins():
    out = subprocess.check_output(["nm", "-C", pkg.library_path()], text=True)
    for name in ("tpp::launch_bf16_chain_widths(", "tpp::plan_chain_widths("):
        kinds = {line.split()[1] for line in out.splitlines() if name in line and len(line.split()) >= 3}
        assert kinds and kinds <= {"T", "t"}, (name, kinds)
