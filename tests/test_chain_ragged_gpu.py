"""Ragged-width bf16 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_ragged) on a real MI355X: with the switch on, a bf16 chain with a
ragged n and / or a layer whose k is a multiple of 8 but not of 64 runs as ONE launch of the chain kernel (brgemm_bf16_lw GRP = 8,
brgemm_bf16_lw_chain_ragged.hip) - rows as under xsmm_hip_set_chain_edge, the last column tile shifted back to end at column n, every batch
element's last chunk shifted back to end at k with its overlap skipped in half steps, the ring carried from layer to layer.

For tile t = 0 .. 3 - (BM, BN) = (32, 64), (64, 64), (64, 128), (128, 128), forced with set_edge_tiles(20 + t) - and the B images VNNI-2, flat
and VNNI-4 (the 64x128 tile has no VNNI-2 instance in this mode - it would need scratch -: such a chain runs on the smallest tile that fits
instead, and the tests read the tile off the counter): m in {BM + 8, 3 BM - 3}; n in {BN + 8, 2 BN + 24} (the later layers have k = n, a
half-step k), n = BN + 16 (a whole-step ragged k), on the 128-wide tiles n = 192 (a whole k with a ragged n); layer 0 takes k from {72, 80,
88, 96, 104, 112, 120, 200} - every skip count 1 .. 7 -, one chain with three batch elements of k = 200 (12 chunks: more than any ring and no
multiple of one), one chain per tile with two batch elements in every layer, one with three ragged layers after a whole-k layer 0 (k = 128).
Every buffer has 8 guard rows behind row m and 8 gap columns beyond its last column: NaN around the layer-0 input, the weights and the bias
rows, a bit pattern around the outputs - checked after every run.
  1 exact inputs, bias + relu: every layer bit for bit the oracle's (the oracle = the fp64 result rounded once, asserted per layer), one
    launch, the new counter up by one, chain_edge_stats and the single-call edge counters unmoved
  2 random operands, six steps on NaN-refilled outputs: the bits of the same calls made one by one on the same tile under set_edge_tiles /
    set_edge_k_bf16 / set_edge_k8_bf16 (20 + t) with the new switch off - the same k-values in the same order, one rounding: exact equality
  3 the windows (part of every case above, and once on m = 4 BM + 5, n = 3 BN + 8: interior and shifted tiles on both axes)
  4 call by call with the bits of the switch-off run: the switch off with the three single-call switches on, strict mode (a process of its
    own), an f32 chain, n % 8 != 0, k % 8 == 4, k < 64, m < BM, a forced generic kernel, synchronous mode, calls that differ in n
  5 with the new switch on a divisible chain runs the plain chain kernel, a ragged-m-only chain runs under set_chain_edge(1) as before and
    call by call without it - the digests of the switch-off run
  6 ShardedMlp(MlpSpec(batch=200, layers=[200, 200, 200, 200])): last_step_fused with the switch on, not with it off, the same bits; and
    layers=[784, 200, 200, 200]
No test tries to provoke a starved or timed-out launch. Every case resets all switches."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chain_edge_worker import BASE, BF16, F32, TILE, RaggedChain, digest
from test_chain_edge_gpu import check_exact
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K0 = [72, 80, 88, 96, 104, 112, 120, 200]  # layer 0: 7, 6, 5, 4, 3, 2, 1 and 7 skipped half steps


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def all_off(rt):
    rt.set_chain_ragged(0), rt.set_chain_edge(0), rt.set_chain_rounds(0), rt.set_edge_tiles(0), rt.set_edge_k_bf16(0), rt.set_edge_k8_bf16(0)


@pytest.fixture()
def rag(rt):
    """asynchronous mode for the case; whatever happens, every switch is 0 afterwards"""
    was_async = rt.set_async(True)
    all_off(rt)
    try:
        yield rt
    finally:
        rt.synchronize()
        all_off(rt)
        rt.set_async(was_async)


def launch_tile(t, image):
    """the tile a chain forced to tile t runs on: t, but for the one instance the mode does not have (64x128, VNNI-2) - there the smallest
    tile, which fits every shape of this file"""
    return 0 if (t == 2 and image == 2) else t


def edge_counters(rt):
    return (rt.chain_edge_stats(), rt.chain_rounds_stats(), rt.edge_tiles_stats(), rt.edge_k_bf16_stats(), rt.edge_k8_bf16_stats())


def run_one_launch(rt, ch, t, outs):
    """the chain through xsmm_hip_fused_brgemm_chain_invoke with the switch on and tile t forced: one launch, counted, nothing else counted"""
    bm, bn = TILE[launch_tile(t, ch.image)]
    all_off(rt)
    rt.set_edge_tiles(20 + t), rt.set_chain_ragged(1)
    before, others = rt.chain_ragged_stats(), edge_counters(rt)
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    rt.synchronize()
    after = rt.chain_ragged_stats()
    assert ran, "xsmm_hip_fused_brgemm_chain_invoke returned 0: the ragged-width chain ran call by call"
    assert after == (before[0] + 1, -(-ch.m // bm), -(-ch.n // bn), BASE[ch.image] + launch_tile(t, ch.image)), (before, after)
    assert edge_counters(rt) == others, "another ragged counter moved"


def separate_calls(rt, ch, t):
    """the same calls one by one on the tile the one launch runs on, under the three single-call switches, the new switch off"""
    all_off(rt)
    f = 20 + launch_tile(t, ch.image)
    rt.set_edge_tiles(f), rt.set_edge_k_bf16(f), rt.set_edge_k8_bf16(f)
    outs = ch.outputs()
    before = rt.chain_ragged_stats()
    ch.one_by_one(outs)
    got = ch.host(outs)
    assert rt.chain_ragged_stats() == before
    return got


def chains(rt, t, image, seed, exact):
    """the chains of tile t: (m, n, ks, brs)"""
    bm, bn = TILE[t]
    k0 = lambda i: K0[(2 * t + i) % len(K0)]
    specs = [(bm + 8, bn + 8, [k0(0), bn + 8, bn + 8], [1, 1, 1]),
             (3 * bm - 3, 2 * bn + 24, [k0(1), 2 * bn + 24, 2 * bn + 24], [1, 1, 1]),
             (bm + 8, bn + 16, [k0(4), bn + 16, bn + 16], [1, 1, 1]),
             (3 * bm - 3, bn + 8, [200, bn + 8, bn + 8], [3, 1, 1]),                         # 12 chunks in layer 0
             (3 * bm - 3, 2 * bn + 16, [k0(5), bn + 8, bn + 8], [2, 2, 2]),                   # two batch elements in every layer
             (bm + 8, bn + 8, [128, bn + 8, bn + 8, bn + 8], [1, 1, 1, 1])]                   # a whole-k layer 0, three ragged layers
    if bn == 128:
        specs.append((bm + 8, 192, [k0(6), 192, 192], [1, 1, 1]))                            # a whole k with a ragged n
    return [RaggedChain(rt, image, m, n, ks, brs, seed + i, exact=exact) for i, (m, n, ks, brs) in enumerate(specs)]


def test_layer_0_takes_every_skip_count():
    seen = set()
    for t in range(4):
        seen |= {(64 - K0[(2 * t + i) % len(K0)] % 64) // 8 for i in ((0, 1, 4, 5, 6) if TILE[t][1] == 128 else (0, 1, 4, 5))}
    assert seen >= set(range(1, 8)), seen


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_one_launch_bit_for_bit_against_the_oracle(rag, t, image):
    for ch in chains(rag, t, image, 1000 * t + 100 * image, exact=True):
        outs = ch.outputs()
        run_one_launch(rag, ch, t, outs)
        got = ch.host(outs)
        ch.check_windows(got)
        check_exact(ch, got)


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_six_steps_have_the_bits_of_the_separate_calls(rag, t, image):
    for ch in chains(rag, t, image, 5000 + 1000 * t + 100 * image, exact=False):
        want = separate_calls(rag, ch, t)
        outs = ch.outputs()
        for step in range(6):
            ch.refill(outs)  # NaN inside, the sentinel around: a stale element of an earlier step cannot pass
            run_one_launch(rag, ch, t, outs)
            got = ch.host(outs)
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[l]), "m %d n %d ks %s step %d layer %d: %d elements differ from the separate calls" % (
                    ch.m, ch.n, ch.ks, step, l, int((got[l] != want[l]).sum()))
        assert np.abs(orc.bf16_to_f32(want[-1].reshape(ch.m + 8, -1)[:ch.m, :ch.n].copy().reshape(-1))).max() > 0


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_windows_with_interior_and_shifted_tiles_on_both_axes(rag, t):
    bm, bn = TILE[t]
    n = 3 * bn + 8
    ch = RaggedChain(rag, 4 if t == 2 else 2, 4 * bm + 5, n, [200, n, n], [1, 1, 1], 40 + t)
    outs = ch.outputs()
    run_one_launch(rag, ch, t, outs)
    got = ch.host(outs)
    ch.check_windows(got)
    want = separate_calls(rag, ch, t)
    for l in range(ch.L):
        assert np.array_equal(got[l], want[l]), "layer %d" % l


def stays_call_by_call(rt, ch, settings, reference, windows=True):
    """under `settings` the chain invoke returns 0 and moves no chain counter; its bits are those of `reference`"""
    all_off(rt)
    settings()
    before = (rt.chain_ragged_stats(), rt.chain_edge_stats())
    outs = ch.outputs()
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    got = ch.host(outs)
    assert not ran, "ran as one launch"
    assert (rt.chain_ragged_stats(), rt.chain_edge_stats()) == before
    if windows:
        ch.check_windows(got)
    for l in range(ch.L):
        assert np.array_equal(got[l], reference[l], equal_nan=ch.dtype == F32), "layer %d" % l


def singles(rt, f):
    rt.set_edge_tiles(f), rt.set_edge_k_bf16(f), rt.set_edge_k8_bf16(f)


def reference_switch_off(rt, ch, f):
    """the calls one by one with the new switch off: under the three single-call switches at f, or under f() if it is a function"""
    all_off(rt)
    f() if callable(f) else singles(rt, f)
    outs = ch.outputs()
    ch.one_by_one(outs)
    return ch.host(outs)


def on(rt, f):
    return lambda: (singles(rt, f), rt.set_chain_ragged(1))


def test_the_switch_off_with_the_single_call_switches_on_stays_call_by_call(rag):
    ch = RaggedChain(rag, 2, 72, 72, [200, 72, 72], [1, 1, 1], 61)
    ref = reference_switch_off(rag, ch, 21)
    stays_call_by_call(rag, ch, lambda: singles(rag, 21), ref)
    run_one_launch(rag, ch, 1, ch.outputs())  # (and the same chain IS taken once the switch is on)


def test_an_f32_chain_stays_call_by_call(rag):
    ch = RaggedChain(rag, 0, 72, 72, [200, 72, 72], [1, 1, 1], 62, dtype=F32)
    ref = reference_switch_off(rag, ch, lambda: rag.set_edge_tiles(2))
    stays_call_by_call(rag, ch, lambda: (rag.set_edge_tiles(2), rag.set_chain_ragged(1)), ref)


def test_n_not_a_multiple_of_8_stays_call_by_call(rag):
    ch = RaggedChain(rag, 2, 72, 68, [192, 64, 64], [1, 1, 1], 63)  # n = BN + 4 (the later layers read the first 64 columns)
    ref = reference_switch_off(rag, ch, 21)
    stays_call_by_call(rag, ch, on(rag, 21), ref)


def test_k_4_mod_8_stays_call_by_call(rag):
    ch = RaggedChain(rag, 2, 72, 72, [76, 72, 72], [1, 1, 1], 64)
    ref = reference_switch_off(rag, ch, 21)
    stays_call_by_call(rag, ch, on(rag, 21), ref)


def test_k_below_64_stays_call_by_call(rag):
    ch = RaggedChain(rag, 2, 72, 72, [56, 72, 72], [1, 1, 1], 65)
    ref = reference_switch_off(rag, ch, 21)
    stays_call_by_call(rag, ch, on(rag, 21), ref)


def test_m_below_every_tile_stays_call_by_call(rag):
    ch = RaggedChain(rag, 2, 24, 72, [200, 72, 72], [1, 1, 1], 66)
    ref = reference_switch_off(rag, ch, 20)
    stays_call_by_call(rag, ch, on(rag, 20), ref)


def test_a_forced_generic_kernel_stays_call_by_call(rag):
    ch = RaggedChain(rag, 2, 72, 72, [200, 72, 72], [1, 1, 1], 67, force=8)
    ref = reference_switch_off(rag, ch, 21)
    stays_call_by_call(rag, ch, on(rag, 21), ref)


def test_synchronous_mode_stays_call_by_call(rag):
    ch = RaggedChain(rag, 2, 72, 72, [200, 72, 72], [1, 1, 1], 68)
    ref = reference_switch_off(rag, ch, 21)
    try:
        stays_call_by_call(rag, ch, lambda: (on(rag, 21)(), rag.set_async(False)), ref)
    finally:
        rag.set_async(True)


def test_calls_that_differ_in_n_stay_call_by_call(rag):
    """the last call has 64 columns where the others have 72: it leaves columns 64 .. 71 of its output as they were, so the windows are
    not asked for - the bits of the switch-off run are"""
    ch = RaggedChain(rag, 2, 72, 72, [200, 72, 72], [1, 1, 1], 69)
    ch.handles[2] = rag.fused_brgemm_dispatch(BF16, 72, 64, 72, ch.ld_in[2], ch.ldb, ch.ldc, 72, 72 * ch.ldb, 4 | 2048, 0, 5, 4, 1)
    ref = reference_switch_off(rag, ch, 21)
    stays_call_by_call(rag, ch, on(rag, 21), ref, windows=False)


@pytest.mark.parametrize("t,image", [(1, 2), (3, 0)])
def test_strict_mode_stays_call_by_call(rag, t, image):
    bm, bn = TILE[t]
    m, n, seed = 3 * bm - 3, bn + 8, 70 + t
    ch = RaggedChain(rag, image, m, n, [200, n, n], [1, 1, 1], seed)
    want = separate_calls(rag, ch, t)
    all_off(rag)
    # strict mode is chosen before anything is queued: a fresh child process (the switches and the tile arrive through the environment there)
    drop = ("TPP_HIP_STRICT", "TPP_HIP_EDGE_TILES", "TPP_HIP_EDGE_K_BF16", "TPP_HIP_EDGE_K8_BF16", "TPP_HIP_CHAIN_EDGE", "TPP_HIP_CHAIN_RAGGED", "TPP_HIP_CHAIN",
            "TPP_HIP_VNNI_FACTOR")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_EDGE_TILES=str(20 + t), TPP_HIP_EDGE_K_BF16=str(20 + t), TPP_HIP_EDGE_K8_BF16=str(20 + t), TPP_HIP_CHAIN_RAGGED="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_ragged_worker.py")] + [str(x) for x in (t, image, m, n, seed)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["chain_ragged_from_env"] == 1 and d["edge_tiles_from_env"] == 20 + t
    assert d["ran_as_one"] is False and d["chain_ragged_stats"][0] == 0
    assert d["digests"] == [digest(w) for w in want], "strict mode runs the calls one by one on the forced tile: the same bits"


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_a_divisible_chain_runs_on_the_chain_kernel_as_before(rag, t):
    bm, bn = TILE[t]
    ch = RaggedChain(rag, 2, 2 * bm, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 80 + t)
    seen = {}
    for sw in (0, 1):
        all_off(rag)
        rag.set_chain_ragged(sw), rag.set_edge_tiles(20 + t)
        before = (rag.chain_ragged_stats(), rag.chain_edge_stats())
        outs = ch.outputs()
        ran = rag.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        ch.check_windows(got)
        assert (rag.chain_ragged_stats(), rag.chain_edge_stats()) == before, "a divisible chain moved a ragged-chain counter"
        seen[sw] = (ran, [digest(g) for g in got])
    assert seen[0][0] is True and seen[1] == seen[0], seen


@pytest.mark.parametrize("t", [1, 3])
def test_a_ragged_m_only_chain_is_the_chain_edge_switch_s(rag, t):
    bm, bn = TILE[t]
    ch = RaggedChain(rag, 2, 3 * bm - 3, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 90 + t)
    seen = {}
    for ragged_sw, edge_sw in ((0, 0), (1, 0), (0, 1), (1, 1)):
        all_off(rag)
        rag.set_chain_ragged(ragged_sw), rag.set_chain_edge(edge_sw), rag.set_edge_tiles(20 + t)
        before, edge_before = rag.chain_ragged_stats(), rag.chain_edge_stats()
        outs = ch.outputs()
        ran = rag.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        ch.check_windows(got)
        assert rag.chain_ragged_stats() == before, "a chain ragged in m alone moved the ragged-width counter"
        assert ran == bool(edge_sw) and rag.chain_edge_stats()[0] == edge_before[0] + edge_sw
        seen[(ragged_sw, edge_sw)] = [digest(g) for g in got]
    assert len({tuple(v) for v in seen.values()}) == 1, seen


def mlp_problem(spec, seed=5):
    import torch
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(spec.batch, spec.layers[0], generator=g) * 0.5).to(torch.bfloat16).cuda()
    Wv, Bs = [], []
    for k, n in zip(spec.layers[:-1], spec.layers[1:]):
        w = (torch.randn(k, n, generator=g) * 0.06).to(torch.bfloat16)
        Wv.append(w.view(k // 2, 2, n).transpose(1, 2).contiguous().cuda())  # VNNI-2 [k / 2][n][2]
        Bs.append((torch.randn(n, generator=g) * 0.1).to(torch.bfloat16).cuda())
    return X, Wv, Bs


@pytest.mark.parametrize("layers", [[200, 200, 200, 200], [784, 200, 200, 200]])
def test_sharded_mlp_fuses_a_200_wide_step_with_the_switch_on(rag, layers):
    """the 64x64 tile forced for the calls and for the launch (the tile decides the order of the sums: the 32x64 tile splits k over two wave
    groups), so the step has the same bits either way"""
    import torch
    spec = pkg.MlpSpec(batch=200, layers=layers)
    X, Wv, Bs = mlp_problem(spec)
    seen = {}
    for sw in (0, 1):
        all_off(rag)
        singles(rag, 21), rag.set_chain_ragged(sw)
        before = rag.chain_ragged_stats()
        mlp = pkg.ShardedMlp(spec, 0, 1, rag)
        acts = [torch.full((spec.batch, n), float("nan"), dtype=torch.bfloat16, device="cuda") for n in spec.layers[1:]]
        mlp.forward(X, Wv, Bs, acts)
        rag.synchronize()
        assert bool(mlp.last_step_fused) == bool(sw), "switch %d" % sw
        assert rag.chain_ragged_stats()[0] == before[0] + sw
        if sw:
            assert rag.chain_ragged_stats()[1:] == (4, 4, 21)
        assert not torch.isnan(acts[-1].float()).any() and acts[-1].float().abs().max() > 0
        seen[sw] = [digest(a.cpu().view(torch.int16).numpy()) for a in acts]
    assert seen[0] == seen[1], "the step as one launch and call by call differ"


def test_the_setter_takes_0_and_1_only(rag):
    assert rag.set_chain_ragged(1) == 0 and rag.set_chain_ragged(0) == 1
    for bad in (-1, 2, 20, 21, 1001):
        assert rag.set_chain_ragged(bad) == -1 and rag.set_chain_ragged(0) == 0
    assert len(rag.chain_ragged_stats()) == 4
