"""Mixed-width bf16 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_widths) on a real MI355X: with the switch on, a bf16 chain whose
layers differ in n runs as ONE launch of the chain kernel (brgemm_bf16_lw GRP = 9, brgemm_bf16_lw_chain_widths.hip) on m / BM x max_l(n_l / BN)
workgroups; workgroup (tm, tn) computes tile (tm, tn) of every layer with a column tile tn and sits out the others.

Buffers as in chain_edge_worker.RaggedChain with per-layer n, ldb and ldc (chain_widths_worker.WidthsChain): 8 guard rows and 8 gap columns
around everything, NaN around the inputs, a sentinel around the outputs, checked after every run. For tile t = 0 .. 3 - (BM, BN) = (32, 64),
(64, 64), (64, 128), (128, 128) - and the B images VNNI-2, flat and VNNI-4, all calls dispatched under force_variant(BASE[image] + t) so that the
launch and the separate calls share the tile; m = 2 BM; layer 0 takes k = 192 (three chunks) unless said otherwise; width vectors
  [3 BN, BN, 2 BN]       a workgroup sits out layer 1 and resumes
  [BN, 3 BN, BN]         first active layer > 0, and a last active layer that is not the chain's last and must signal
  [4 BN, 2 BN, BN]       a funnel
  [2 BN, BN] * 4         eight layers
  [2 BN, 2 BN, BN]       two batch elements per layer (k = n_prev / 2; layer 0 two of 192)
  [256, 128, 256]        k0 = 128: every chunk count even - tiles 0 and 1 run two chunks per barrier
  [2 BN, BN]             three batch elements of k = 256 in layer 0 (12 chunks: more than any ring)
  1 exact inputs, bias + relu: every layer bit for bit the oracle's, one launch, the counter up by one with the row blocks, the widest
    layer's column tiles and the variant; no other chain counter and no single-call counter moved
  2 random operands, six steps on refilled outputs: exact equality with the same calls made one by one with the switch off
  3 [3 BN, BN, 3 BN] and [BN, 3 BN, 3 BN] - one grid and layer count, different inner widths - alternate three times each on one stream
  4 call by call with the bits of the switch-off run: the switch off, an f32 chain, calls that differ in m, a ragged m under
    set_chain_edge(1), an n_l no tile's columns divide, a k of 200 under set_chain_ragged(1), synchronous mode, strict mode with calls
    dispatched on different tiles (a process of its own)
  5 with the switch on an equal-width chain runs the plain chain kernel and a ragged-width equal-n chain runs under set_chain_ragged(1) as
    before: the same digests, no counter of this mode moved
  6 ShardedMlp(MlpSpec(batch=256, layers=[256, 512, 128, 256])) under force_variant(21): last_step_fused with the switch on, not with it
    off, the same bits
No test tries to provoke a starved or timed-out launch. Every case resets all switches."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chain_edge_worker import BASE, BF16, F32, TILE, RaggedChain, digest
from chain_widths_worker import WidthsChain, check_exact

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def all_off(rt):
    rt.set_chain_widths(0), rt.set_chain_ragged(0), rt.set_chain_edge(0), rt.set_chain_rounds(0)
    rt.set_edge_tiles(0), rt.set_edge_k_bf16(0), rt.set_edge_k8_bf16(0)
    rt.force_variant(-1)


@pytest.fixture()
def wid(rt):
    """asynchronous mode for the case; whatever happens, every switch is 0 afterwards"""
    was_async = rt.set_async(True)
    all_off(rt)
    try:
        yield rt
    finally:
        rt.synchronize()
        all_off(rt)
        rt.set_async(was_async)


def other_counters(rt):
    return (rt.chain_edge_stats(), rt.chain_rounds_stats(), rt.chain_ragged_stats(), rt.edge_tiles_stats(), rt.edge_k_bf16_stats(), rt.edge_k8_bf16_stats())


def run_one_launch(rt, ch, t, outs):
    """the chain through xsmm_hip_fused_brgemm_chain_invoke with the switch on: one launch, counted, nothing else counted"""
    bm, bn = TILE[t]
    all_off(rt)
    rt.set_chain_widths(1)
    before, others = rt.chain_widths_stats(), other_counters(rt)
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    rt.synchronize()
    after = rt.chain_widths_stats()
    assert ran, "xsmm_hip_fused_brgemm_chain_invoke returned 0: the mixed-width chain ran call by call"
    assert after == (before[0] + 1, ch.m // bm, max(ch.ns) // bn, BASE[ch.image] + t), (before, after)
    assert other_counters(rt) == others, "another chain or single-call counter moved"


def separate_calls(rt, ch):
    """the same calls one by one (dispatched on the same tile) with the switch off"""
    all_off(rt)
    outs = ch.outputs()
    before = rt.chain_widths_stats()
    ch.one_by_one(outs)
    got = ch.host(outs)
    assert rt.chain_widths_stats() == before
    return got


def specs(t):
    """(ns, ks, brs) of tile t's chains"""
    bn = TILE[t][1]
    chain = lambda ns, k0=192: (ns, [k0] + ns[:-1], [1] * len(ns))
    return [chain([3 * bn, bn, 2 * bn]), chain([bn, 3 * bn, bn]), chain([4 * bn, 2 * bn, bn]), chain([2 * bn, bn] * 4),
            ([2 * bn, 2 * bn, bn], [192, bn, bn], [2, 2, 2]),
            chain([256, 128, 256], k0=128),
            ([2 * bn, bn], [256, 2 * bn], [3, 1])]


def chains(rt, t, image, seed, exact):
    return [WidthsChain(rt, image, 2 * TILE[t][0], ns, ks, brs, seed + i, exact=exact, tiles=t) for i, (ns, ks, brs) in enumerate(specs(t))]


def test_the_width_vectors_cover_the_schedule_s_cases():
    for t in range(4):
        bn = TILE[t][1]
        tiles = [[n // bn for n in ns] for ns, _, _ in specs(t)]
        assert all(n % bn == 0 for ns, _, _ in specs(t) for n in ns)
        assert any(any(a > b < c for a, b, c in zip(v, v[1:], v[2:])) for v in tiles), "a workgroup sits out a layer and resumes"
        assert any(v[0] < max(v) and v[-1] < max(v) for v in tiles), "first active layer > 0 and a non-final last active layer"
        assert any(len(v) == 8 for v in tiles)
        chunks = [[b * (k // 64) for k, b in zip(ks, brs)] for _, ks, brs in specs(t)]
        assert any(all(c % 2 == 0 for c in cs) for cs in chunks) and any(cs[0] % 2 == 1 for cs in chunks) and any(cs[0] == 12 for cs in chunks)


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_one_launch_bit_for_bit_against_the_oracle(wid, t, image):
    for ch in chains(wid, t, image, 1000 * t + 100 * image, exact=True):
        outs = ch.outputs()
        run_one_launch(wid, ch, t, outs)
        got = ch.host(outs)
        ch.check_windows(got)
        check_exact(ch, got)


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_six_steps_have_the_bits_of_the_separate_calls(wid, t, image):
    for ch in chains(wid, t, image, 5000 + 1000 * t + 100 * image, exact=False):
        want = separate_calls(wid, ch)
        outs = ch.outputs()
        for step in range(6):
            ch.refill(outs)  # NaN inside, the sentinel around: a stale element of an earlier step cannot pass
            run_one_launch(wid, ch, t, outs)
            got = ch.host(outs)
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[l]), "m %d ns %s step %d layer %d: %d elements differ from the separate calls" % (
                    ch.m, ch.ns, step, l, int((got[l] != want[l]).sum()))
        assert (want[-1].reshape(ch.m + 8, -1)[:ch.m, :ch.ns[-1]] & 0x7fff).max() > 0


@pytest.mark.parametrize("t,image", [(0, 2), (1, 0), (2, 4), (3, 2)])
def test_two_chains_with_one_grid_and_different_inner_widths_alternate_on_one_stream(wid, t, image):
    bm, bn = TILE[t]
    a = WidthsChain(wid, image, 2 * bm, [3 * bn, bn, 3 * bn], [192, 3 * bn, bn], [1, 1, 1], 300 + t, tiles=t)
    b = WidthsChain(wid, image, 2 * bm, [bn, 3 * bn, 3 * bn], [192, bn, 3 * bn], [1, 1, 1], 310 + t, tiles=t)
    want = {id(ch): separate_calls(wid, ch) for ch in (a, b)}
    outs = {id(ch): ch.outputs() for ch in (a, b)}
    for step in range(3):
        for ch in (a, b):
            ch.refill(outs[id(ch)])
            run_one_launch(wid, ch, t, outs[id(ch)])
            got = ch.host(outs[id(ch)])
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[id(ch)][l]), "ns %s step %d layer %d" % (ch.ns, step, l)


def chain_counters(rt):
    return (rt.chain_widths_stats(), rt.chain_edge_stats(), rt.chain_rounds_stats(), rt.chain_ragged_stats())


def stays_call_by_call(rt, ch, settings, reference, rows=None):
    """under `settings` the chain invoke returns 0 and moves no chain counter; its bits are those of `reference`"""
    all_off(rt)
    settings()
    before = chain_counters(rt)
    outs = ch.outputs()
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    got = ch.host(outs)
    assert not ran, "ran as one launch"
    assert chain_counters(rt) == before
    ch.check_windows(got, rows)
    for l in range(ch.L):
        assert np.array_equal(got[l], reference[l], equal_nan=ch.dtype == F32), "layer %d" % l


def reference_switch_off(rt, ch, settings=lambda: None):
    all_off(rt)
    settings()
    outs = ch.outputs()
    ch.one_by_one(outs)
    return ch.host(outs)


def test_the_switch_off_stays_call_by_call_and_the_same_chain_is_taken_with_it_on(wid):
    ch = WidthsChain(wid, 2, 128, [192, 64, 128], [192, 192, 64], [1, 1, 1], 61, tiles=1)
    ref = reference_switch_off(wid, ch)
    stays_call_by_call(wid, ch, lambda: None, ref)
    outs = ch.outputs()
    run_one_launch(wid, ch, 1, outs)
    got = ch.host(outs)
    for l in range(ch.L):
        assert np.array_equal(got[l], ref[l])


def test_an_f32_chain_stays_call_by_call(wid):
    ch = WidthsChain(wid, 0, 128, [192, 64, 128], [192, 192, 64], [1, 1, 1], 62, dtype=F32)
    ref = reference_switch_off(wid, ch)
    stays_call_by_call(wid, ch, lambda: wid.set_chain_widths(1), ref)


def test_calls_that_differ_in_m_stay_call_by_call(wid):
    """the last call has 64 rows where the others have 128: it leaves rows 64 .. 127 of its output as they were"""
    ch = WidthsChain(wid, 2, 128, [192, 64, 128], [192, 192, 64], [1, 1, 1], 63, tiles=1, ms=[128, 128, 64])
    ref = reference_switch_off(wid, ch)
    stays_call_by_call(wid, ch, lambda: wid.set_chain_widths(1), ref, rows=[128, 128, 64])


def test_a_ragged_m_stays_call_by_call_under_the_chain_edge_switch(wid):
    ch = WidthsChain(wid, 2, 125, [192, 64, 128], [192, 192, 64], [1, 1, 1], 64)
    ref = reference_switch_off(wid, ch, lambda: wid.set_edge_tiles(21))
    stays_call_by_call(wid, ch, lambda: (wid.set_edge_tiles(21), wid.set_chain_edge(1), wid.set_chain_widths(1)), ref)


def test_an_n_no_tile_divides_stays_call_by_call(wid):
    """n_1 = 96: 96 % 64 != 0 and 96 % 128 != 0 (layer 2 reads its first 64 columns)"""
    ch = WidthsChain(wid, 2, 128, [128, 96, 128], [192, 128, 64], [1, 1, 1], 65)
    ref = reference_switch_off(wid, ch, lambda: wid.set_edge_tiles(21))
    stays_call_by_call(wid, ch, lambda: (wid.set_edge_tiles(21), wid.set_chain_ragged(1), wid.set_chain_widths(1)), ref)


def test_a_k_of_200_stays_call_by_call_under_the_chain_ragged_switch(wid):
    ch = WidthsChain(wid, 2, 128, [128, 64, 128], [200, 128, 64], [1, 1, 1], 66)
    singles = lambda: (wid.set_edge_tiles(21), wid.set_edge_k_bf16(21), wid.set_edge_k8_bf16(21))
    ref = reference_switch_off(wid, ch, singles)
    stays_call_by_call(wid, ch, lambda: (singles(), wid.set_chain_ragged(1), wid.set_chain_widths(1)), ref)


def test_synchronous_mode_stays_call_by_call(wid):
    ch = WidthsChain(wid, 2, 128, [192, 64, 128], [192, 192, 64], [1, 1, 1], 67, tiles=1)
    ref = reference_switch_off(wid, ch)
    try:
        stays_call_by_call(wid, ch, lambda: (wid.set_chain_widths(1), wid.set_async(False)), ref)
    finally:
        wid.set_async(True)


def test_strict_mode_with_calls_dispatched_on_different_tiles_stays_call_by_call(wid):
    image, m, seed, ns, tiles = 2, 128, 68, [256, 128, 256], [1, 2, 1]
    ch = WidthsChain(wid, image, m, ns, [192] + ns[:-1], [1, 1, 1], seed, tiles=tiles)
    want = separate_calls(wid, ch)
    all_off(wid)
    # strict mode is chosen before anything is queued: a fresh child process (the switch arrives through the environment there)
    drop = ("TPP_HIP_STRICT", "TPP_HIP_EDGE_TILES", "TPP_HIP_EDGE_K_BF16", "TPP_HIP_EDGE_K8_BF16", "TPP_HIP_CHAIN_EDGE", "TPP_HIP_CHAIN_RAGGED", "TPP_HIP_CHAIN_ROUNDS",
            "TPP_HIP_CHAIN_WIDTHS", "TPP_HIP_CHAIN", "TPP_HIP_VNNI_FACTOR")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_CHAIN_WIDTHS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_widths_worker.py"), str(image), str(m), str(seed), ",".join(map(str, ns)), ",".join(map(str, tiles))],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["chain_widths_from_env"] == 1
    assert d["ran_as_one"] is False and d["chain_widths_stats"][0] == 0
    assert d["digests"] == [digest(w) for w in want], "strict mode runs the calls one by one on their own tiles: the same bits"


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_an_equal_width_chain_runs_on_the_plain_chain_kernel_as_before(wid, t):
    bm, bn = TILE[t]
    ch = WidthsChain(wid, 2, 2 * bm, [2 * bn] * 3, [192, 2 * bn, 2 * bn], [1, 1, 1], 80 + t, tiles=t)
    seen = {}
    for sw in (0, 1):
        all_off(wid)
        wid.set_chain_widths(sw)
        before = chain_counters(wid)
        outs = ch.outputs()
        ran = wid.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        ch.check_windows(got)
        assert chain_counters(wid) == before, "an equal-width chain moved a counter of the opt-in chain modes"
        seen[sw] = (ran, [digest(g) for g in got])
    assert seen[0][0] is True and seen[1] == seen[0], seen


def test_a_ragged_width_equal_n_chain_is_the_chain_ragged_switch_s(wid):
    ch = RaggedChain(wid, 2, 72, 72, [200, 72, 72], [1, 1, 1], 90)
    seen = {}
    for sw in (0, 1):
        all_off(wid)
        wid.set_edge_tiles(21), wid.set_chain_ragged(1), wid.set_chain_widths(sw)
        before, ragged_before = wid.chain_widths_stats(), wid.chain_ragged_stats()
        outs = ch.outputs()
        ran = wid.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        ch.check_windows(got)
        assert ran and wid.chain_ragged_stats()[0] == ragged_before[0] + 1 and wid.chain_widths_stats() == before
        seen[sw] = [digest(g) for g in got]
    assert seen[0] == seen[1]


def test_sharded_mlp_fuses_a_mixed_width_step_with_the_switch_on(wid):
    """the 64x64 tile forced for the calls, which the launch then takes: the step has the same bits either way"""
    import torch
    spec = pkg.MlpSpec(batch=256, layers=[256, 512, 128, 256])
    g = torch.Generator().manual_seed(5)
    X = (torch.randn(spec.batch, spec.layers[0], generator=g) * 0.5).to(torch.bfloat16).cuda()
    Wv, Bs = [], []
    for k, n in zip(spec.layers[:-1], spec.layers[1:]):
        w = (torch.randn(k, n, generator=g) * 0.06).to(torch.bfloat16)
        Wv.append(w.view(k // 2, 2, n).transpose(1, 2).contiguous().cuda())  # VNNI-2 [k / 2][n][2]
        Bs.append((torch.randn(n, generator=g) * 0.1).to(torch.bfloat16).cuda())
    seen = {}
    for sw in (0, 1):
        all_off(wid)
        wid.set_chain_widths(sw)
        before = wid.chain_widths_stats()
        wid.force_variant(21)
        try:
            mlp = pkg.ShardedMlp(spec, 0, 1, wid)
            acts = [torch.full((spec.batch, n), float("nan"), dtype=torch.bfloat16, device="cuda") for n in spec.layers[1:]]
            mlp.forward(X, Wv, Bs, acts)
        finally:
            wid.force_variant(-1)
        wid.synchronize()
        assert bool(mlp.last_step_fused) == bool(sw), "switch %d" % sw
        assert wid.chain_widths_stats()[0] == before[0] + sw
        if sw:
            assert wid.chain_widths_stats()[1:] == (4, 8, 21)
        assert not torch.isnan(acts[-1].float()).any() and acts[-1].float().abs().max() > 0
        seen[sw] = [digest(a.cpu().view(torch.int16).numpy()) for a in acts]
    assert seen[0] == seen[1], "the step as one launch and call by call differ"
