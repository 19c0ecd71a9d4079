"""CPU-side checks of the ragged mixed-width chain switch (include/tpp_xsmm_abi.h xsmm_hip_set_chain_widths_ragged /
xsmm_hip_chain_widths_ragged_stats): the header declares both symbols, the library exports them, tpp-mlir_amd/runtime.py wraps them and
lists their signatures, the setter takes 0 and 1 only and returns the previous mode, TPP_HIP_CHAIN_WIDTHS_RAGGED is read, the counters
start at zero - and the weak stand-ins that let the host-only builds of runtime.cpp link are where the real definitions override them."""
import importlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("tpp-mlir_amd")
SYMBOLS = ("xsmm_hip_set_chain_widths_ragged", "xsmm_hip_chain_widths_ragged_stats")
ENV = "TPP_HIP_CHAIN_WIDTHS_RAGGED"


@pytest.fixture(scope="module")
def rt():
    pkg.build()
    return pkg.get_runtime()


def test_the_header_declares_and_the_library_exports_both_symbols(rt):
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        declared = re.findall(r"TPP_XSMM_EXPORT\s+[\w\s\*]+?\b(\w+)\s*\(", f.read())
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    runtime_py = importlib.import_module("tpp-mlir_amd.runtime")
    for s in SYMBOLS:
        assert s in declared and s in exported and hasattr(rt.lib, s) and s in runtime_py._SIGNATURES, s
    assert callable(rt.set_chain_widths_ragged) and callable(rt.chain_widths_ragged_stats)


def test_the_setter_takes_0_and_1_only_and_returns_the_previous_mode(rt):
    first = rt.set_chain_widths_ragged(0)
    assert first in (0, 1)
    try:
        assert rt.set_chain_widths_ragged(1) == 0 and rt.set_chain_widths_ragged(1) == 1 and rt.set_chain_widths_ragged(0) == 1
        for bad in (-1, 2, 11, 20, 23, 1001):
            assert rt.set_chain_widths_ragged(bad) == -1, bad
            assert rt.set_chain_widths_ragged(0) == 0, "a refused value changed the mode"
        assert rt.set_chain_widths(2) == -1 and rt.set_chain_ragged(2) == -1 and rt.set_chain_edge(2) == -1, "the other chain switches still take 0 and 1 only"
        stats = rt.chain_widths_ragged_stats()
        assert len(stats) == 4 and all(isinstance(v, int) for v in stats) and stats[0] >= 0
    finally:
        rt.set_chain_widths_ragged(first)


def _fresh(env_value):
    """(stats, previous mode) in a process of its own"""
    env = {k: v for k, v in os.environ.items() if k != ENV}
    if env_value is not None:
        env[ENV] = env_value
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(rt.chain_widths_ragged_stats(), rt.set_chain_widths_ragged(0), rt.set_chain_widths(0), rt.set_chain_ragged(0))" % ROOT)
    return subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]


def test_the_counters_start_at_zero_and_the_switch_is_off_by_default():
    assert _fresh(None) == "(0, 0, 0, 0) 0 0 0"


def test_the_environment_variable_is_read_and_turns_no_other_switch_on():
    assert _fresh("1") == "(0, 0, 0, 0) 1 0 0"
    assert _fresh("2") == "(0, 0, 0, 0) 0 0 0", "a value the setter refuses leaves the switch off"


def test_the_real_planner_and_launcher_override_the_weak_stand_ins():
    out = subprocess.check_output(["nm", "-C", pkg.library_path()], text=True)
    for name in ("tpp::launch_bf16_chain_wragged(", "tpp::plan_chain_widths_ragged(", "tpp::chain_widths_ragged_b_kind("):
        kinds = {line.split()[1] for line in out.splitlines() if name in line and len(line.split()) >= 3}
        assert kinds and kinds <= {"T", "t"}, (name, kinds)
