"""The eighteen opt-in mode switches of the C-ABI (include/tpp_xsmm_abi.h xsmm_hip_set_<name> / xsmm_hip_<name>_stats), all of them, on the
CPU: the header declares both symbols, the library exports them, tpp-mlir_amd/runtime.py wraps them; the setter returns the previous mode
for every accepted value and -1, with the mode unchanged, for every other; setting one switch moves no other; the counter count agrees
between the header, the Python wrapper and the library; TPP_HIP_<NAME> is read when the library is loaded and a refused value leaves the
default. The table below is the specification, written out: nothing in it is taken from the code under test."""
import ctypes
import importlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("tpp-mlir_amd")
rtmod = importlib.import_module("tpp-mlir_amd.runtime")

UP_TO_16 = frozenset(range(0, 17))
UP_TO_2 = frozenset(range(0, 3))
ON_OFF = frozenset((0, 1))
BF16_TILES = frozenset((0, 1, 20, 21, 22, 23))
BN = frozenset((0, 1, 16, 32, 64))
FORCED_GROUPS = frozenset((0, 1)) | frozenset(range(1001, 66537))  # 1000 + G, 1 <= G <= 0x10000

# name: (accepted values, counters of the stats block, default, two accepted values other than the default for the environment test)
SWITCHES = {
    "tail_split": (UP_TO_16, 4, 0, (1, 16)),
    "edge_tiles": (frozenset((0, 1, 2, 6, 7, 9, 10, 20, 21, 22, 23)), 4, 0, (2, 23)),
    "edge_k": (frozenset((0, 1, 6, 7, 9, 10)), 4, 0, (1, 10)),
    "edge_k_bf16": (BF16_TILES, 4, 0, (1, 23)),
    "edge_k8_bf16": (BF16_TILES, 4, 0, (20, 22)),
    "dma256_images": (UP_TO_2, 4, 0, (1, 2)),
    "dma256_edge": (UP_TO_2, 4, 0, (2, 1)),
    "skinny_bf16": (BN, 5, 0, (1, 64)),
    "skinny_split": (UP_TO_16, 3, 0, (16, 2)),
    "f32_halves": (UP_TO_2, 4, 1, (0, 2)),
    "chain_edge": (ON_OFF, 4, 0, (1, 1)),
    "chain_rounds": (FORCED_GROUPS, 4, 0, (1, 66536)),
    "chain_ragged": (ON_OFF, 4, 0, (1, 1)),
    "chain_widths": (ON_OFF, 4, 0, (1, 1)),
    "chain_width_rounds": (FORCED_GROUPS, 4, 0, (1001, 1)),
    "chain_widths_ragged": (ON_OFF, 4, 0, (1, 1)),
    "chain_dma256": (FORCED_GROUPS | frozenset((2,)), 4, 0, (2, 1016)),
    "chain_skinny": (BN | frozenset(1000 * g + bn for g in range(1, 513) for bn in (16, 32, 64)), 4, 0, (32, 512064)),
}
NAMES = tuple(SWITCHES)
# what every setter is asked: both ends of every range of the table, values inside, and the neighbours just outside
PROBES = (list(range(-2, 70)) + list(range(995, 1070)) + [1999, 2000, 2015, 2016, 2017, 2032, 2064, 2065, 30000, 65535, 65536, 65537]
          + list(range(66530, 66540)) + [255016, 255064, 511064, 512000, 512015, 512016, 512017, 512032, 512033, 512064, 512065,
                                         513000, 513016, 513032, 513064, 1000016, 2 ** 31 - 1, -2 ** 31])


def env_name(name):
    return "TPP_HIP_" + name.upper()


@pytest.fixture(scope="module")
def rt():
    pkg.build()
    return pkg.get_runtime()


def mode_of(rt, name):
    """the switch's mode (there is no getter: a setter returns the previous one), left as it was"""
    setter = getattr(rt, "set_" + name)
    mode = setter(SWITCHES[name][2])
    assert setter(mode) == SWITCHES[name][2]
    return mode


def test_the_table_has_eighteen_rows_and_probes_both_sides_of_every_row():
    assert len(SWITCHES) == 18
    for name, (accepted, n, default, env_values) in SWITCHES.items():
        assert default in accepted and all(v in accepted and v != default for v in env_values), name
        assert min(accepted) == 0 and {min(accepted) - 1, max(accepted) + 1, max(accepted)} <= set(PROBES), name
        assert len(accepted & set(PROBES)) >= 2 and len(set(PROBES) - accepted) >= 6, name


@pytest.mark.parametrize("name", NAMES)
def test_the_header_declares_the_library_exports_and_the_runtime_wraps_both_symbols(rt, name):
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        declared = re.findall(r"TPP_XSMM_EXPORT\s+[\w\s\*]+?\b(\w+)\s*\(", f.read())
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in ("xsmm_hip_set_" + name, "xsmm_hip_" + name + "_stats"):
        assert s in declared and s in exported and hasattr(rt.lib, s) and s in rtmod._SIGNATURES, s
    assert rtmod._SIGNATURES["xsmm_hip_set_" + name] == (ctypes.c_int, [ctypes.c_int])
    assert rtmod._SIGNATURES["xsmm_hip_" + name + "_stats"] == (None, [ctypes.POINTER(ctypes.c_int64)])
    for method in ("set_" + name, name + "_stats"):
        assert callable(getattr(rt, method)) and getattr(type(rt), method).__doc__, method


@pytest.mark.parametrize("name", NAMES)
def test_the_setter_returns_the_previous_mode_or_refuses_and_changes_nothing(rt, name):
    accepted = SWITCHES[name][0]
    setter = getattr(rt, "set_" + name)
    first = mode_of(rt, name)
    assert first in accepted
    try:
        prev = first
        for v in PROBES:
            got = setter(v)
            assert type(got) is int
            if v in accepted:
                assert got == prev, (v, got, prev)
                prev = v
            else:
                assert got == -1, (v, got)
                assert mode_of(rt, name) == prev, "the refused value %d changed the mode" % v
    finally:
        setter(first)
    assert mode_of(rt, name) == first


def test_setting_one_switch_leaves_the_other_seventeen_unchanged(rt):
    before = {name: mode_of(rt, name) for name in NAMES}
    for name in NAMES:
        for value in SWITCHES[name][3]:
            assert getattr(rt, "set_" + name)(value) in SWITCHES[name][0]
            for other in NAMES:
                if other != name:
                    assert mode_of(rt, other) == before[other], (name, value, other)
        getattr(rt, "set_" + name)(before[name])
    assert {name: mode_of(rt, name) for name in NAMES} == before


@pytest.mark.parametrize("name", NAMES)
def test_the_counter_count_agrees_in_the_header_the_wrapper_and_the_library(rt, name):
    n = SWITCHES[name][1]
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        sizes = re.findall(r"TPP_XSMM_EXPORT\s+void\s+xsmm_hip_%s_stats\s*\(\s*int64_t\s+out\[(\d+)\]\s*\)" % name, f.read())
    assert sizes == [str(n)], sizes
    stats = getattr(rt, name + "_stats")()
    assert type(stats) is tuple and len(stats) == n and all(type(v) is int and v >= 0 for v in stats), stats
    # the library itself: every one of the n words is written, the word behind them is not
    sentinel = -0x5EED5EED5EED
    buf = (ctypes.c_int64 * (n + 1))(*([sentinel] * (n + 1)))
    getattr(rt.lib, "xsmm_hip_%s_stats" % name)(buf)
    assert buf[n] == sentinel, "the library wrote past %d words" % n
    assert tuple(buf[:n]) == stats, (tuple(buf), stats)


def children(env_values):
    """ONE child process that reports (counters, mode) of all eighteen switches; env_values: name -> the variable's text (absent: unset)"""
    env = {k: v for k, v in os.environ.items() if k not in {env_name(n) for n in NAMES}}
    env.update({env_name(n): v for n, v in env_values.items()})
    code = ("import importlib, json, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(json.dumps({n: [list(getattr(rt, n + '_stats')()), getattr(rt, 'set_' + n)(0)] for n in %r}))" % (ROOT, list(NAMES)))
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1]
    return json.loads(out)


@pytest.fixture(scope="module")
def built():
    pkg.build()


@pytest.mark.parametrize("which", ("unset", "refused", "accepted", "accepted again"))
def test_the_environment_variables_are_read_in_a_child_process(built, which):
    """processes of their own: no launch has been counted; without its variable, or with a value its setter refuses, a switch has its
    default; with an accepted value it has that value - all eighteen at once, each variable read by its own switch alone"""
    if which == "unset":
        env, want = {}, {n: SWITCHES[n][2] for n in NAMES}
    elif which == "refused":
        env = {n: str(max(SWITCHES[n][0]) + 1 if i % 2 else -1) for i, n in enumerate(NAMES)}
        want = {n: SWITCHES[n][2] for n in NAMES}
    else:
        want = {n: SWITCHES[n][3][which == "accepted again"] for n in NAMES}
        env = {n: str(v) for n, v in want.items()}
    got = children(env)
    assert sorted(got) == sorted(NAMES)
    for n in NAMES:
        assert got[n] == [[0] * SWITCHES[n][1], want[n]], (n, env.get(n), got[n])
