"""CPU-side checks of the column-round switch (include/tpp_xsmm_abi.h xsmm_hip_set_chain_width_rounds / xsmm_hip_chain_width_rounds_stats): the
header declares both symbols, the library exports them, tpp-mlir_amd/runtime.py wraps them, the setter takes 0, 1 and 1000 + W (W >= 1) and
returns the previous mode, the environment variable is read as a number, the counters start at zero - and the weak stand-ins that let the
host-only builds of runtime.cpp link are where the real definitions override them."""
import importlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("tpp-mlir_amd")
SYMBOLS = ("xsmm_hip_set_chain_width_rounds", "xsmm_hip_chain_width_rounds_stats")


@pytest.fixture(scope="module")
def rt():
    pkg.build()
    return pkg.get_runtime()


def test_the_header_declares_and_the_library_exports_both_symbols(rt):
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        declared = re.findall(r"TPP_XSMM_EXPORT\s+[\w\s\*]+?\b(\w+)\s*\(", f.read())
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    rtmod = importlib.import_module("tpp-mlir_amd.runtime")
    for s in SYMBOLS:
        assert s in declared and s in exported and hasattr(rt.lib, s) and s in rtmod._SIGNATURES, s


def test_the_setter_takes_0_1_and_a_forced_w_and_returns_the_previous_mode(rt):
    first = rt.set_chain_width_rounds(0)
    assert first == 0 or first == 1 or first > 1000
    try:
        assert rt.set_chain_width_rounds(1) == 0 and rt.set_chain_width_rounds(1) == 1 and rt.set_chain_width_rounds(1001) == 1
        assert rt.set_chain_width_rounds(1016) == 1001 and rt.set_chain_width_rounds(0) == 1016
        for bad in (2, -1, 1000, 999):
            assert rt.set_chain_width_rounds(bad) == -1, bad
            assert rt.set_chain_width_rounds(0) == 0, "a refused value changed the mode"
        assert rt.set_chain_widths(2) == -1 and rt.set_chain_widths(1001) == -1, "xsmm_hip_set_chain_widths still takes 0 and 1 only"
        stats = rt.chain_width_rounds_stats()
        assert len(stats) == 4 and all(isinstance(v, int) for v in stats) and stats[0] >= 0
    finally:
        rt.set_chain_width_rounds(first)


def child(env_value):
    env = {k: v for k, v in os.environ.items() if k != "TPP_HIP_CHAIN_WIDTH_ROUNDS"}
    if env_value is not None:
        env["TPP_HIP_CHAIN_WIDTH_ROUNDS"] = env_value
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(rt.chain_width_rounds_stats(), rt.set_chain_width_rounds(0), rt.set_chain_widths(0))" % ROOT)
    return subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]


def test_the_counters_start_at_zero_and_the_switch_is_off_by_default():
    """a process of its own: no launch has been counted, and without the environment variable the mode is 0"""
    assert child(None) == "(0, 0, 0, 0) 0 0"


@pytest.mark.parametrize("value,mode", [("1", 1), ("1016", 1016), ("0", 0), ("2", 0), ("1000", 0), ("-1", 0), ("on", 0)])
def test_the_environment_variable_is_read_as_a_number_in_a_child_process(value, mode):
    """... and sets this switch alone; a value the setter would refuse leaves it off"""
    assert child(value) == "(0, 0, 0, 0) %d 0" % mode


def test_the_real_planner_and_launcher_override_the_weak_stand_ins():
    out = subprocess.check_output(["nm", "-C", pkg.library_path()], text=True)
    for name in ("tpp::launch_bf16_chain_wrounds(", "tpp::plan_chain_width_rounds("):
        kinds = {line.split()[1] for line in out.splitlines() if name in line and len(line.split()) >= 3}
        assert kinds and kinds <= {"T", "t"}, (name, kinds)
