"""Multi-round bf16 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_rounds) on a real MI355X: with the switch on, a bf16 chain runs as
ONE launch of the chain kernel on G resident row groups (brgemm_bf16_lw GRP = 7) - workgroup (g, tn) walks the row blocks g, g + G, .. of
every layer, layer-major, and waits at every seam for the counter of the row block it is about to read.

For tile t = 0 .. 3 - (BM, BN) = (32, 64), (64, 64), (64, 128), (128, 128), forced at dispatch as tests/test_chain_gpu.py forces it, so that
the chain takes the planned tile - and mode 1000 + G the shapes are (chain_rounds_worker.shapes): 5 BM x 2 BN on G = 2 (uneven: the groups
own 3 and 2 row blocks), 4 BM x BN on G = 2 (even), 3 BM x 2 BN on G = 1 (one group walks every block), 3 BM on G = 2 with n = k =
64 x NSLOT in every layer (the B loaders run ahead across steps), 5 BM x 2 BN on G = 2 with two batch elements per layer and stride_a along
k. Three layers, bias + relu; layer 0 has k = 192 where the shape does not say otherwise. B images VNNI-2, flat and VNNI-4. Every buffer
has 8 guard rows behind row m and 8 gap columns beyond its last column: NaN around the layer-0 input, the weights and the bias rows, a bit
pattern around the outputs - checked after every run.
  1 exact inputs: every layer bit for bit the oracle's, one launch, the stats (count + 1, G, ceil(tiles_m / G), variant), neither the
    chain-edge nor the edge-tile counters move
  2 random operands, six steps on NaN-refilled outputs: the bits of the same calls made one by one on the same tile with the switch off
  3 mode 1 on a real overflow: tile 0, n = 64, m = 32 x (CUs + 8), k = 64, 64, 64 - the rule gives R = 2; bits as in 2; and the gate:
    three rounds stay call by call under mode 1, a forced G takes them
  4 as with the switch off - its bits, its return value, unmoved stats: the switch off, a chain that fits under mode 1, a ragged m, f32,
    synchronous mode, a forced G >= tiles_m
  5 strict mode in a process of its own: one launch on the planned tile, the bits of the strict separate calls
Every case resets the switch to 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chain_edge_worker import BASE, BF16, F32, TILE, RaggedChain, digest
from chain_rounds_worker import make, shapes
from oracle import pyoracle as orc
from test_chain_edge_gpu import check_exact

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture()
def rounds(rt):
    """asynchronous mode for the case; whatever happens, the switch is 0 afterwards"""
    was_async = rt.set_async(True)
    try:
        yield rt
    finally:
        rt.synchronize()
        rt.set_chain_rounds(0)
        rt.set_async(was_async)


def run_one_launch(rt, ch, mode, want_stats, outs):
    """the chain through xsmm_hip_fused_brgemm_chain_invoke under `mode`: one launch, counted with (G, R, variant) = want_stats; neither
    the chain-edge nor the edge-tile counters move"""
    rt.set_chain_rounds(mode)
    before, edge_before, tiles_before = rt.chain_rounds_stats(), rt.chain_edge_stats(), rt.edge_tiles_stats()
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    rt.synchronize()
    after = rt.chain_rounds_stats()
    rt.set_chain_rounds(0)
    assert ran, "xsmm_hip_fused_brgemm_chain_invoke returned 0: the chain ran call by call"
    assert after == (before[0] + 1,) + tuple(want_stats), (before, after)
    assert rt.chain_edge_stats() == edge_before and rt.edge_tiles_stats() == tiles_before, "a ragged-chain or edge-tile launch was counted"


def stats_of(t, image, shape):
    m, _, _, _, G = shape
    return (G, -(-(m // TILE[t][0]) // G), BASE[image] + t)


def separate_calls_switch_off(rt, ch):
    """the same calls one by one on the tile forced at dispatch, the switch off"""
    rt.set_chain_rounds(0)
    outs = ch.outputs()
    ch.one_by_one(outs)
    got = ch.host(outs)
    ch.check_windows(got)
    return got


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_one_launch_bit_for_bit_against_the_oracle(rounds, t, image):
    for i, shape in enumerate(shapes(t)):
        ch = make(rounds, t, image, shape, 1000 + 100 * t + 10 * image + i, exact=True)
        outs = ch.outputs()
        run_one_launch(rounds, ch, 1000 + shape[4], stats_of(t, image, shape), outs)
        got = ch.host(outs)
        ch.check_windows(got)
        check_exact(ch, got)


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_six_steps_have_the_bits_of_the_separate_calls(rounds, t, image):
    for i, shape in enumerate(shapes(t)):
        ch = make(rounds, t, image, shape, 2000 + 100 * t + 10 * image + i)
        want = separate_calls_switch_off(rounds, ch)
        outs = ch.outputs()
        for step in range(6):
            ch.refill(outs)  # NaN inside, the sentinel around: a stale element of an earlier step cannot pass
            run_one_launch(rounds, ch, 1000 + shape[4], stats_of(t, image, shape), outs)
            got = ch.host(outs)
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[l]), "shape %d step %d layer %d: %d elements differ from the separate calls" % (i, step, l, int((got[l] != want[l]).sum()))
        m, n = shape[0], shape[1]
        assert np.abs(orc.bf16_to_f32(want[-1].reshape(m + 8, -1)[:m, :n].copy().reshape(-1))).max() > 0


def overflow_chain(rt, seed):
    """tile 0 forced, one column tile, 8 row blocks more than the device has compute units: the smallest chain that does not fit"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus, RaggedChain(rt, 2, 32 * (cus + 8), 64, [64, 64, 64], [1, 1, 1], seed, force=BASE[2] + 0)


def test_mode_1_runs_a_chain_that_overflows_the_compute_units_in_two_rounds(rounds):
    cus, ch = overflow_chain(rounds, 31)
    want = separate_calls_switch_off(rounds, ch)
    outs = ch.outputs()
    for step in range(6):
        ch.refill(outs)
        run_one_launch(rounds, ch, 1, (-(-(cus + 8) // 2), 2, BASE[2] + 0), outs)  # Gmax = CUs: R = 2, G = ceil((CUs + 8) / 2)
        got = ch.host(outs)
        ch.check_windows(got)
        for l in range(ch.L):
            assert np.array_equal(got[l], want[l]), "step %d layer %d: %d elements differ from the separate calls" % (step, l, int((got[l] != want[l]).sum()))


def as_with_the_switch_off(rt, ch, mode, call_by_call=None, settings=None):
    """under `mode` the chain invoke does what it does with the switch off: the same return value (call_by_call: and that value is 0),
    the same bits - those of the calls one by one - and no multi-round launch is counted"""
    want = separate_calls_switch_off(rt, ch)
    seen = {}
    for sw in (0, mode):
        rt.set_chain_rounds(sw)
        if settings:
            settings()
        before = rt.chain_rounds_stats()
        outs = ch.outputs()
        ran = bool(rt.fused_brgemm_chain(ch.dtype, ch.calls(outs)))
        got = ch.host(outs)
        assert rt.chain_rounds_stats() == before, "a multi-round launch was counted"
        ch.check_windows(got)
        for l in range(ch.L):
            assert np.array_equal(got[l], want[l], equal_nan=ch.dtype == F32), "switch %d layer %d" % (sw, l)
        seen[sw] = ran
    rt.set_chain_rounds(0)
    assert seen[mode] == seen[0], seen
    if call_by_call is not None:
        assert seen[mode] is (not call_by_call), seen


def test_the_switch_off_leaves_an_overflowing_chain_call_by_call(rounds):
    # CUs + 9 row blocks of 32 rows - an odd number -, one column tile: too many tiles of 32x64, and no larger tile divides the rows
    # (a flat B: the one-round rules take an odd number of 32-row blocks of it, of VNNI-2 they ask for 64 rows)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ch = RaggedChain(rounds, 0, 32 * (cus + 9), 64, [64, 64, 64], [1, 1, 1], 41, force=BASE[0] + 0)
    as_with_the_switch_off(rounds, ch, 0, call_by_call=True)
    # (and the same chain IS taken once the switch is on: two rounds)
    run_one_launch(rounds, ch, 1, (-(-(cus + 9) // 2), 2, BASE[0] + 0), ch.outputs())


def test_the_gate_leaves_three_rounds_call_by_call_and_a_forced_g_takes_them(rounds):
    """2 CUs + 1 row blocks: three rounds. Mode 1 takes at most two (measured: deeper chains were slower than the separate calls); a
    forced G is not gated and has the bits of the separate calls"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ch = RaggedChain(rounds, 0, 32 * (2 * cus + 1), 64, [64, 64, 64], [1, 1, 1], 47, force=BASE[0] + 0)
    as_with_the_switch_off(rounds, ch, 1, call_by_call=True)
    want = separate_calls_switch_off(rounds, ch)
    g = -(-(2 * cus + 1) // 3)
    outs = ch.outputs()
    run_one_launch(rounds, ch, 1000 + g, (g, 3, BASE[0] + 0), outs)
    got = ch.host(outs)
    ch.check_windows(got)
    for l in range(ch.L):
        assert np.array_equal(got[l], want[l]), "layer %d: %d elements differ from the separate calls" % (l, int((got[l] != want[l]).sum()))


def test_a_chain_that_fits_runs_on_the_chain_kernel_under_mode_1(rounds):
    ch = make(rounds, 1, 2, shapes(1)[0], 42)
    as_with_the_switch_off(rounds, ch, 1, call_by_call=False)


def test_a_ragged_m_stays_call_by_call(rounds):
    ch = RaggedChain(rounds, 2, 5 * 64 + 8, 128, [192, 128, 128], [1, 1, 1], 43, force=BASE[2] + 1)
    as_with_the_switch_off(rounds, ch, 1002, call_by_call=True)
    as_with_the_switch_off(rounds, ch, 1, call_by_call=True)


def test_an_f32_chain_is_left_alone(rounds):
    ch = RaggedChain(rounds, 0, 5 * 64, 128, [192, 128, 128], [1, 1, 1], 44, dtype=F32)
    as_with_the_switch_off(rounds, ch, 1002)
    as_with_the_switch_off(rounds, ch, 1)


def test_synchronous_mode_stays_call_by_call(rounds):
    ch = make(rounds, 1, 2, shapes(1)[0], 45)
    try:
        as_with_the_switch_off(rounds, ch, 1002, call_by_call=True, settings=lambda: rounds.set_async(False))
    finally:
        rounds.set_async(True)


@pytest.mark.parametrize("g", [3, 4])
def test_a_forced_g_of_tiles_m_or_more_changes_nothing(rounds, g):
    ch = make(rounds, 1, 0, shapes(1)[2], 46)  # three row blocks
    as_with_the_switch_off(rounds, ch, 1000 + g)


@pytest.mark.parametrize("t,image,index", [(1, 2, 0), (3, 0, 4), (0, 2, 0)])
def test_strict_mode_takes_the_rule_on_the_planned_tile(rounds, t, image, index):
    shape, seed = shapes(t)[index], 50 + t
    # strict mode is chosen before anything is queued: a fresh child process (the switch arrives through the environment there)
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_STRICT", "TPP_HIP_EDGE_TILES", "TPP_HIP_CHAIN_EDGE", "TPP_HIP_CHAIN_ROUNDS", "TPP_HIP_CHAIN", "TPP_HIP_VNNI_FACTOR")}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_CHAIN_ROUNDS=str(1000 + shape[4]))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_rounds_worker.py")] + [str(x) for x in (t, image, index, seed)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["chain_rounds_from_env"] == 1000 + shape[4]
    assert d["ran_as_one"] is True and d["chain_rounds_stats"] == [1] + list(stats_of(t, image, shape)), d
    assert d["chain_edge_launches"] == 0 and d["edge_tiles_launches"] == 0
    assert d["digests"] == d["separate"], "one launch on the planned tile: the bits of the strict separate calls"


def test_the_setter_takes_0_1_and_forced_groups_only(rounds):
    assert rounds.set_chain_rounds(1) == 0 and rounds.set_chain_rounds(1002) == 1 and rounds.set_chain_rounds(0) == 1002
    for bad in (-1, 2, 20, 999, 1000):
        assert rounds.set_chain_rounds(bad) == -1 and rounds.set_chain_rounds(0) == 0
    assert len(rounds.chain_rounds_stats()) == 4
