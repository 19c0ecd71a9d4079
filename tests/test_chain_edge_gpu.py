"""Ragged-m bf16 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_edge) on a real MI355X: with the switch on, a bf16 chain whose m the
tile's rows do not divide runs as ONE launch of the chain kernel on edge row tiles (brgemm_bf16_lw GRP = 5) - the last row block shifted
back to end at row m, storing its own rows only, waiting at every seam for both row blocks whose rows it reads.

For tile t = 0 .. 3 - (BM, BN) = (32, 64), (64, 64), (64, 128), (128, 128), forced with set_edge_tiles(20 + t) - the shapes are
m in {BM + 8, 3 BM - 3} x n in {BN, 2 BN}: two row blocks with the last owning 8 rows; three row blocks, so that the last block waits for
blocks 1 and 2 and not for block 0 (the single-layer edge tiles take an odd m: 3 BM - 3 it is). Three layers: layer 0 has k = 192 in one
batch element (three chunks), the later ones k = n; one further chain per tile has two batch elements in every layer, stride_a along k.
B images VNNI-2, flat and VNNI-4. Every buffer has 8 guard rows behind row m and 8 gap columns beyond its last column: NaN around the
layer-0 input, the weights and the bias rows, a bit pattern around the outputs - checked after every run.
  1 exact inputs, bias + relu: every layer bit for bit the oracle's, one launch, the launch counter up by one, no edge launch
  2 random operands, six steps on NaN-refilled outputs: the bits of the same three calls made one by one on the same forced tile, switch off
  3 the windows (part of every case above, and once by itself on all-tiles shapes)
  4 call by call with the bits of the switch off: the switch off under mode 2, strict mode (a process of its own), an f32 ragged chain, a
    ragged n, m below every tile, the generic kernel forced, synchronous mode - the counter does not move
  5 a divisible chain (m = 2 BM) with the switch on: today's chain kernel, the counter does not move, the bits of the switch off
No test can force the race the two-counter wait closes; 1 and 2 make it visible when it happens. Every case resets the switch and the
edge-tile mode to 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chain_edge_worker import BASE, BF16, F32, TILE, RaggedChain, digest, make_chain
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture()
def edge(rt):
    """asynchronous mode for the case; whatever happens, the switch and the edge-tile mode are 0 afterwards"""
    was_async = rt.set_async(True)
    try:
        yield rt
    finally:
        rt.synchronize()
        rt.set_chain_edge(0)
        rt.set_edge_tiles(0)
        rt.set_async(was_async)


def shapes(t):
    bm, bn = TILE[t]
    return [(m, n) for m in (bm + 8, 3 * bm - 3) for n in (bn, 2 * bn)]


def run_one_launch(rt, ch, t, outs):
    """the chain through xsmm_hip_fused_brgemm_chain_invoke with the switch on and tile t forced: one launch, counted, no edge launch"""
    bm, bn = TILE[t]
    rt.set_edge_tiles(20 + t), rt.set_chain_edge(1)
    before, edge_before = rt.chain_edge_stats(), rt.edge_tiles_stats()
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    rt.synchronize()
    after = rt.chain_edge_stats()
    assert ran, "xsmm_hip_fused_brgemm_chain_invoke returned 0: the ragged chain ran call by call"
    assert after == (before[0] + 1, -(-ch.m // bm), ch.n // bn, BASE[ch.image] + t), (before, after)
    assert rt.edge_tiles_stats() == edge_before, "a single-layer edge launch was made"


def check_exact(ch, got):
    """every layer bit for bit the oracle's (fed the oracle's previous layer), the exactness precondition checked per layer: the oracle's
    output is the fp64 result rounded once"""
    ref, prev = ch.oracle(), ch.x
    v = ch.image or 1
    for l in range(ch.L):
        K = ch.ks[l] * ch.brs[l]
        rows = ch.m + 8
        xin = orc.bf16_to_f32(prev).reshape(rows, -1)[:ch.m, :K].astype(np.float64)
        w = orc.bf16_to_f32(ch.W[l]).reshape(-1, ch.ldb, v)[:K // v, :ch.n, :].transpose(0, 2, 1).reshape(K, ch.n).astype(np.float64)
        f64 = np.maximum(xin @ w + orc.bf16_to_f32(ch.b[l])[:ch.n].astype(np.float64)[None, :], 0)
        r2, g2 = ref[l].reshape(rows, ch.ldc), got[l].reshape(rows, ch.ldc)
        assert np.array_equal(orc.f32_to_bf16(f64.astype(np.float32).reshape(-1)).reshape(ch.m, ch.n), r2[:ch.m, :ch.n]), "layer %d not exact" % l
        bad = g2 != r2
        assert not bad.any(), "layer %d: %d elements differ from the oracle, first at (row, column) %s" % (l, int(bad.sum()), tuple(np.argwhere(bad)[0]))
        prev = ref[l]


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_one_launch_bit_for_bit_against_the_oracle(edge, t, image):
    for i, (m, n) in enumerate(shapes(t)):
        ch = make_chain(edge, t, image, m, n, 100 * t + 10 * image + i, exact=True)
        outs = ch.outputs()
        run_one_launch(edge, ch, t, outs)
        got = ch.host(outs)
        ch.check_windows(got)
        check_exact(ch, got)


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_two_batch_elements_per_layer(edge, t, image):
    bm, bn = TILE[t]
    ch = make_chain(edge, t, image, 3 * bm - 3, 2 * bn, 500 + 10 * t + image, br2=True, exact=True)
    outs = ch.outputs()
    run_one_launch(edge, ch, t, outs)
    got = ch.host(outs)
    ch.check_windows(got)
    check_exact(ch, got)


def separate_calls_switch_off(rt, ch, t):
    """the same calls one by one, tile t forced, the switch off: every one an edge launch on that tile"""
    rt.set_chain_edge(0), rt.set_edge_tiles(20 + t)
    outs = ch.outputs()
    before = rt.edge_tiles_stats()
    ch.one_by_one(outs)
    got = ch.host(outs)
    assert rt.edge_tiles_stats()[0] == before[0] + ch.L and rt.edge_tiles_stats()[3] == BASE[ch.image] + t
    return got


@pytest.mark.parametrize("br2", [False, True], ids=["br1", "br2"])
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_six_steps_have_the_bits_of_the_separate_calls(edge, t, image, br2):
    bm, bn = TILE[t]
    for m, n in ([(3 * bm - 3, 2 * bn)] if br2 else [(bm + 8, 2 * bn), (3 * bm - 3, bn)]):
        ch = make_chain(edge, t, image, m, n, 900 + 10 * t + image, br2=br2)
        want = separate_calls_switch_off(edge, ch, t)
        outs = ch.outputs()
        for step in range(6):
            ch.refill(outs)  # NaN inside, the sentinel around: a stale element of an earlier step cannot pass
            run_one_launch(edge, ch, t, outs)
            got = ch.host(outs)
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[l]), "step %d layer %d: %d elements differ from the separate calls" % (step, l, int((got[l] != want[l]).sum()))
        assert np.abs(orc.bf16_to_f32(want[-1].reshape(m + 8, -1)[:m, :n].copy().reshape(-1))).max() > 0


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_windows_with_every_tile_row_and_column_in_use(edge, t):
    """five row blocks, three column tiles: interior blocks, a shifted last block, guards on every side"""
    bm, bn = TILE[t]
    ch = make_chain(edge, t, 2, 4 * bm + 5, 3 * bn, 40 + t)
    outs = ch.outputs()
    run_one_launch(edge, ch, t, outs)
    got = ch.host(outs)
    ch.check_windows(got)
    want = separate_calls_switch_off(edge, ch, t)
    for l in range(ch.L):
        assert np.array_equal(got[l], want[l]), "layer %d" % l


def stays_call_by_call(rt, ch, settings, reference):
    """under `settings` (applied with the switch ON unless they say otherwise) the chain invoke returns 0 and moves no counter; its bits are
    those of `reference` (the same calls with the switch off)"""
    settings()
    before = rt.chain_edge_stats()
    outs = ch.outputs()
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    got = ch.host(outs)
    assert not ran, "ran as one launch"
    assert rt.chain_edge_stats() == before
    ch.check_windows(got)
    for l in range(ch.L):
        assert np.array_equal(got[l], reference[l], equal_nan=ch.dtype == F32), "layer %d" % l


def reference_switch_off(rt, ch, mode):
    rt.set_chain_edge(0), rt.set_edge_tiles(mode)
    outs = ch.outputs()
    ch.one_by_one(outs)
    return ch.host(outs)


def test_the_switch_off_under_mode_2_stays_call_by_call(edge):
    ch = make_chain(edge, 1, 2, 189, 128, 61)
    ref = reference_switch_off(edge, ch, 2)
    stays_call_by_call(edge, ch, lambda: (edge.set_chain_edge(0), edge.set_edge_tiles(2)), ref)
    run_one_launch(edge, ch, 1, ch.outputs())  # (and the same chain IS taken once the switch is on)


def test_an_f32_ragged_chain_stays_call_by_call(edge):
    ch = RaggedChain(edge, 0, 189, 128, [192, 128, 128], [1, 1, 1], 62, dtype=F32)
    ref = reference_switch_off(edge, ch, 2)
    stays_call_by_call(edge, ch, lambda: (edge.set_chain_edge(1), edge.set_edge_tiles(2)), ref)


def test_a_ragged_n_stays_call_by_call(edge):
    ch = RaggedChain(edge, 2, 189, 136, [192, 128, 128], [1, 1, 1], 63)  # (the later layers read the first 128 of the 136 columns)
    ref = reference_switch_off(edge, ch, 21)
    stays_call_by_call(edge, ch, lambda: (edge.set_chain_edge(1), edge.set_edge_tiles(21)), ref)


def test_m_below_every_tile_stays_call_by_call(edge):
    ch = make_chain(edge, 0, 2, 24, 128, 64)
    ref = reference_switch_off(edge, ch, 20)
    stays_call_by_call(edge, ch, lambda: (edge.set_chain_edge(1), edge.set_edge_tiles(20)), ref)


def test_a_forced_generic_kernel_stays_call_by_call(edge):
    ch = make_chain(edge, 1, 2, 189, 128, 65, force=8)
    ref = reference_switch_off(edge, ch, 21)
    stays_call_by_call(edge, ch, lambda: (edge.set_chain_edge(1), edge.set_edge_tiles(21)), ref)


def test_synchronous_mode_stays_call_by_call(edge):
    ch = make_chain(edge, 1, 2, 189, 128, 66)
    ref = reference_switch_off(edge, ch, 21)
    try:
        stays_call_by_call(edge, ch, lambda: (edge.set_chain_edge(1), edge.set_edge_tiles(21), edge.set_async(False)), ref)
    finally:
        edge.set_async(True)


@pytest.mark.parametrize("t,image", [(1, 2), (3, 0)])
def test_strict_mode_stays_call_by_call(edge, t, image):
    bm, bn = TILE[t]
    m, n, seed = 3 * bm - 3, 2 * bn, 70 + t
    ch = make_chain(edge, t, image, m, n, seed)
    want = separate_calls_switch_off(edge, ch, t)
    edge.set_edge_tiles(0)
    # strict mode is chosen before anything is queued: a fresh child process (the switch and the tile arrive through the environment there)
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_STRICT", "TPP_HIP_EDGE_TILES", "TPP_HIP_CHAIN_EDGE", "TPP_HIP_CHAIN", "TPP_HIP_VNNI_FACTOR")}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_EDGE_TILES=str(20 + t), TPP_HIP_CHAIN_EDGE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_edge_worker.py")] + [str(x) for x in (t, image, m, n, seed)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["chain_edge_from_env"] == 1 and d["edge_tiles_from_env"] == 20 + t
    assert d["ran_as_one"] is False and d["chain_edge_stats"][0] == 0 and d["edge_tiles_launches"] == 3
    assert d["digests"] == [digest(w) for w in want], "strict mode runs the calls one by one on the forced tile: the same bits"


@pytest.mark.parametrize("image", [2, 0])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_a_divisible_chain_runs_on_the_chain_kernel_as_before(edge, t, image):
    bm, bn = TILE[t]
    ch = make_chain(edge, t, image, 2 * bm, 2 * bn, 80 + t)
    seen = {}
    for sw in (0, 1):
        edge.set_chain_edge(sw), edge.set_edge_tiles(20 + t)
        before = edge.chain_edge_stats()
        outs = ch.outputs()
        ran = edge.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        ch.check_windows(got)
        assert edge.chain_edge_stats() == before, "a divisible chain moved the ragged-chain counter"
        seen[sw] = (ran, [digest(g) for g in got])
    assert seen[0][0] is True and seen[1] == seen[0], seen


def test_the_setter_takes_0_and_1_only(edge):
    assert edge.set_chain_edge(1) == 0 and edge.set_chain_edge(0) == 1
    for bad in (-1, 2, 20, 21):
        assert edge.set_chain_edge(bad) == -1 and edge.set_chain_edge(0) == 0
    assert len(edge.chain_edge_stats()) == 4
