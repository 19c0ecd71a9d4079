"""Ragged mixed-width bf16 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_widths_ragged) on a real MI355X: with the switch on, a bf16
chain whose layers differ in n and that no tile divides entirely runs as ONE launch of the chain kernel (brgemm_bf16_lw GRP = 11,
brgemm_bf16_lw_chain_wragged.hip) on ceil(m / BM) x max_l ceil(n_l / BN) workgroups.

Buffers: chain_widths_worker.WidthsChain - 8 guard rows and 8 gap columns around everything, NaN around the inputs, a sentinel around the
outputs, checked after every run. For tile t = 0 .. 3 - (BM, BN) = (32, 64), (64, 64), (64, 128), (128, 128), forced with
set_edge_tiles(20 + t) - and the B images VNNI-2, flat and VNNI-4; the one absent instance (64x128, VNNI-2) lands on the smallest tile,
which the counter shows. The chains (chain_widths_ragged_worker.specs), with m in {BM + 8, 3 BM - 3}:
  [3 BN + 8, BN + 8, 2 BN + 24]     sit out and resume; every layer's last tile shifted; a tile last in one layer, interior in the next
  [BN + 8, 3 BN, BN + 16]           first active layer > 0; whole and ragged widths mixed; k classes half-step, whole and whole-step
  [4 BN, 2 BN, BN]                  k0 from {72, 80, 88, 96, 104, 112, 120, 200}: ragged k only
  [3 BN, BN, 2 BN]                  k0 = 192, m = 3 BM - 3: ragged m only
  [2 BN, BN]                        three batch elements of k = 200 in layer 0: 12 chunks
  [2 BN + 8, BN + 8] * 4            eight layers
  [2 BN + 16, 2 BN + 16, BN + 8]    two batch elements per layer
  1 exact inputs, bias + relu: every layer bit for bit the oracle's, one launch, the new counter up by one with the right [1] .. [3]; no
    other chain counter and no single-call edge counter moved
  2 random operands, six steps on refilled outputs: exact equality with the same calls one by one on the same tile under the three
    single-call switches, the new switch off
  3 windows: m = 4 BM + 5 with widths [3 BN + 8, BN, 2 BN + 8] - interior and shifted tiles on both axes
  4 two chains with one grid and one layer count but different inner widths alternate three times each on one stream
  5 call by call with the bits of the switch-off run: the switch off with the six other switches on, strict mode (a process of its own),
    f32, n % 8 != 0, k % 8 == 4, k < 64, m < BM, some n_l < BN, a forced generic kernel, synchronous mode, calls that differ in m
  6 with the new switch on the existing modes are untouched: mode 9 / call by call for a divisible mixed-width chain, mode 8, mode 5
  7 ShardedMlp fuses a ragged mixed-width step
No test tries to provoke a starved or timed-out launch. Every case resets all switches."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chain_edge_worker import BASE, BF16, F32, TILE, RaggedChain, b_image, digest
from chain_widths_worker import WidthsChain, check_exact
from chain_widths_ragged_worker import K0, launch_tile, specs

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def all_off(rt):
    rt.set_chain_widths_ragged(0), rt.set_chain_widths(0), rt.set_chain_width_rounds(0), rt.set_chain_ragged(0), rt.set_chain_edge(0), rt.set_chain_rounds(0)
    rt.set_edge_tiles(0), rt.set_edge_k_bf16(0), rt.set_edge_k8_bf16(0)
    rt.force_variant(-1)


@pytest.fixture()
def wr(rt):
    """asynchronous mode for the case; whatever happens, every switch is 0 afterwards"""
    was_async = rt.set_async(True)
    all_off(rt)
    try:
        yield rt
    finally:
        rt.synchronize()
        all_off(rt)
        rt.set_async(was_async)


def singles(rt, f):
    rt.set_edge_tiles(f), rt.set_edge_k_bf16(f), rt.set_edge_k8_bf16(f)


def other_counters(rt):
    return (rt.chain_widths_stats(), rt.chain_width_rounds_stats(), rt.chain_edge_stats(), rt.chain_rounds_stats(), rt.chain_ragged_stats(), rt.edge_tiles_stats(),
            rt.edge_k_bf16_stats(), rt.edge_k8_bf16_stats())


def run_one_launch(rt, ch, t, outs):
    """the chain through xsmm_hip_fused_brgemm_chain_invoke with the switch on and tile t forced: one launch, counted, nothing else counted"""
    lt = launch_tile(t, ch.image)
    bm, bn = TILE[lt]
    all_off(rt)
    rt.set_edge_tiles(20 + t), rt.set_chain_widths_ragged(1)
    before, others = rt.chain_widths_ragged_stats(), other_counters(rt)
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    rt.synchronize()
    after = rt.chain_widths_ragged_stats()
    assert ran, "xsmm_hip_fused_brgemm_chain_invoke returned 0: the ragged mixed-width chain ran call by call"
    assert after == (before[0] + 1, -(-ch.m // bm), -(-max(ch.ns) // bn), BASE[ch.image] + lt), (before, after)
    assert other_counters(rt) == others, "another chain or single-call counter moved"


def separate_calls(rt, ch, t):
    """the same calls one by one on the tile the one launch runs on, under the three single-call switches, the new switch off"""
    all_off(rt)
    singles(rt, 20 + launch_tile(t, ch.image))
    outs = ch.outputs()
    before = rt.chain_widths_ragged_stats()
    ch.one_by_one(outs)
    got = ch.host(outs)
    assert rt.chain_widths_ragged_stats() == before
    return got


def chains(rt, t, mi, image, seed, exact):
    return [WidthsChain(rt, image, m, ns, ks, brs, seed + i, exact=exact) for i, (_, m, ns, ks, brs) in enumerate(specs(t, mi))]


def test_the_chains_cover_the_schedule_s_cases():
    for t in range(4):
        bm, bn = TILE[t]
        both = specs(t, 0) + specs(t, 1)
        assert {m for _, m, _, _, _ in both} == {bm + 8, 3 * bm - 3}
        tiles = [[-(-n // bn) for n in ns] for _, _, ns, _, _ in both]
        assert any(any(a > b < c for a, b, c in zip(v, v[1:], v[2:])) for v in tiles), "a workgroup sits out a layer and resumes"
        assert any(v[0] < max(v) and v[-1] < max(v) for v in tiles), "first active layer > 0 and a non-final last active layer"
        assert any(len(v) == 8 for v in tiles)
        assert {ks[0] for _, _, ns, ks, _ in both if ns == [4 * bn, 2 * bn, bn]} == set(K0)
        assert {(64 - k % 64) // 8 for k in K0 if k < 128} == set(range(1, 8)), "every skip count"
        assert any(brs[0] * -(-ks[0] // 64) == 12 for _, _, _, ks, brs in both)
        assert any(m % bm and all(n % bn == 0 for n in ns) and all(k % 64 == 0 for k in ks) for _, m, ns, ks, _ in both), "ragged m only"
        assert any(brs == [2, 2, 2] for _, _, _, _, brs in both)
        for _, m, ns, ks, brs in both:
            assert len(set(ns)) > 1 and all(n % 8 == 0 and n >= bn for n in ns) and all(k % 8 == 0 and k >= 64 for k in ks) and m >= bm
            assert m % bm or any(n % bn for n in ns) or any(k % 64 for k in ks), "no chain the tile divides entirely"


@pytest.mark.parametrize("mi", [0, 1])
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_one_launch_bit_for_bit_against_the_oracle(wr, t, image, mi):
    for ch in chains(wr, t, mi, image, 1000 * t + 100 * image + 10000 * mi, exact=True):
        outs = ch.outputs()
        run_one_launch(wr, ch, t, outs)
        got = ch.host(outs)
        ch.check_windows(got)
        check_exact(ch, got)


@pytest.mark.parametrize("mi", [0, 1])
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_six_steps_have_the_bits_of_the_separate_calls(wr, t, image, mi):
    for ch in chains(wr, t, mi, image, 5000 + 1000 * t + 100 * image + 10000 * mi, exact=False):
        want = separate_calls(wr, ch, t)
        outs = ch.outputs()
        for step in range(6):
            ch.refill(outs)  # NaN inside, the sentinel around: a stale element of an earlier step cannot pass
            run_one_launch(wr, ch, t, outs)
            got = ch.host(outs)
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[l]), "m %d ns %s ks %s step %d layer %d: %d elements differ from the separate calls" % (
                    ch.m, ch.ns, ch.ks, step, l, int((got[l] != want[l]).sum()))
        assert (want[-1].reshape(ch.m + 8, -1)[:ch.m, :ch.ns[-1]] & 0x7fff).max() > 0


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_windows_with_interior_and_shifted_tiles_on_both_axes(wr, t):
    bm, bn = TILE[t]
    ns = [3 * bn + 8, bn, 2 * bn + 8]
    ch = WidthsChain(wr, 4 if t == 2 else 2, 4 * bm + 5, ns, [200] + ns[:-1], [1, 1, 1], 40 + t)
    outs = ch.outputs()
    run_one_launch(wr, ch, t, outs)
    got = ch.host(outs)
    ch.check_windows(got)
    want = separate_calls(wr, ch, t)
    for l in range(ch.L):
        assert np.array_equal(got[l], want[l]), "layer %d" % l


@pytest.mark.parametrize("t,image", [(0, 2), (1, 0), (2, 4), (3, 2)])
def test_two_chains_with_one_grid_and_different_inner_widths_alternate_on_one_stream(wr, t, image):
    """the keyed counter block: layer 0 of a adds 3 to its counters, layer 0 of b adds 1"""
    bm, bn = TILE[t]
    a = WidthsChain(wr, image, bm + 8, [3 * bn - 8, bn + 8, 3 * bn - 8], [136, 3 * bn - 8, bn + 8], [1, 1, 1], 300 + t)
    b = WidthsChain(wr, image, bm + 8, [bn, 3 * bn - 8, 3 * bn - 8], [136, bn, 3 * bn - 8], [1, 1, 1], 310 + t)
    want = {id(ch): separate_calls(wr, ch, t) for ch in (a, b)}
    outs = {id(ch): ch.outputs() for ch in (a, b)}
    for step in range(3):
        for ch in (a, b):
            ch.refill(outs[id(ch)])
            run_one_launch(wr, ch, t, outs[id(ch)])
            got = ch.host(outs[id(ch)])
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[id(ch)][l]), "ns %s step %d layer %d" % (ch.ns, step, l)


def chain_counters(rt):
    return (rt.chain_widths_ragged_stats(), rt.chain_widths_stats(), rt.chain_width_rounds_stats(), rt.chain_edge_stats(), rt.chain_rounds_stats(), rt.chain_ragged_stats())


def stays_call_by_call(rt, ch, settings, reference, rows_=None, windows=True):
    """under `settings` the chain invoke returns 0 and moves no chain counter; its bits are those of `reference`"""
    all_off(rt)
    settings()
    before = chain_counters(rt)
    outs = ch.outputs()
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    got = ch.host(outs)
    assert not ran, "ran as one launch"
    assert chain_counters(rt) == before
    if windows:
        ch.check_windows(got, rows_)
    for l in range(ch.L):
        assert np.array_equal(got[l], reference[l], equal_nan=ch.dtype == F32), "layer %d" % l


def reference_switch_off(rt, ch, f):
    """the calls one by one with the new switch off: under the three single-call switches at f, or under f() if it is a function"""
    all_off(rt)
    f() if callable(f) else singles(rt, f)
    outs = ch.outputs()
    ch.one_by_one(outs)
    return ch.host(outs)


def on(rt, f):
    return lambda: (singles(rt, f), rt.set_chain_widths_ragged(1))


NS, KS = [200, 136, 72], [200, 200, 136]  # the small chain of the refusals: 72 rows on the 64x64 tile


def test_the_switch_off_with_the_six_other_switches_on_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 72, NS, KS, [1, 1, 1], 61)
    ref = reference_switch_off(wr, ch, 21)
    stays_call_by_call(wr, ch, lambda: (singles(wr, 21), wr.set_chain_edge(1), wr.set_chain_ragged(1), wr.set_chain_widths(1)), ref)
    run_one_launch(wr, ch, 1, ch.outputs())  # (and the same chain IS taken once the switch is on)


@pytest.mark.parametrize("t,image", [(1, 2), (3, 0)])
def test_strict_mode_stays_call_by_call(wr, t, image):
    bm, bn = TILE[t]
    m, seed = 3 * bm - 3, 70 + t
    ns = [2 * bn + 8, bn + 8, bn + 16]
    ks = [200] + ns[:-1]
    ch = WidthsChain(wr, image, m, ns, ks, [1, 1, 1], seed)
    want = separate_calls(wr, ch, t)
    all_off(wr)
    # strict mode is chosen before anything is queued: a fresh child process (the switches and the tile arrive through the environment there)
    drop = ("TPP_HIP_STRICT", "TPP_HIP_EDGE_TILES", "TPP_HIP_EDGE_K_BF16", "TPP_HIP_EDGE_K8_BF16", "TPP_HIP_CHAIN_EDGE", "TPP_HIP_CHAIN_RAGGED", "TPP_HIP_CHAIN_ROUNDS",
            "TPP_HIP_CHAIN_WIDTHS", "TPP_HIP_CHAIN_WIDTH_ROUNDS", "TPP_HIP_CHAIN_WIDTHS_RAGGED", "TPP_HIP_CHAIN", "TPP_HIP_VNNI_FACTOR")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_EDGE_TILES=str(20 + t), TPP_HIP_EDGE_K_BF16=str(20 + t), TPP_HIP_EDGE_K8_BF16=str(20 + t), TPP_HIP_CHAIN_WIDTHS_RAGGED="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_widths_ragged_worker.py")] + [str(x) for x in (t, image, m, seed)] +
                       [",".join(map(str, ns)), ",".join(map(str, ks))], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["chain_widths_ragged_from_env"] == 1 and d["edge_tiles_from_env"] == 20 + t
    assert d["ran_as_one"] is False and d["chain_widths_ragged_stats"][0] == 0
    assert d["digests"] == [digest(w) for w in want], "strict mode runs the calls one by one on the forced tile: the same bits"


def test_an_f32_chain_stays_call_by_call(wr):
    ch = WidthsChain(wr, 0, 72, NS, KS, [1, 1, 1], 62, dtype=F32)
    ref = reference_switch_off(wr, ch, lambda: wr.set_edge_tiles(2))
    stays_call_by_call(wr, ch, lambda: (wr.set_edge_tiles(2), wr.set_chain_widths_ragged(1)), ref)


def test_n_not_a_multiple_of_8_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 72, [200, 132, 72], [200, 200, 128], [1, 1, 1], 63)  # n_1 = 132 (layer 2 reads its first 128 columns)
    ref = reference_switch_off(wr, ch, 21)
    stays_call_by_call(wr, ch, on(wr, 21), ref)


def test_k_4_mod_8_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 72, NS, [76, 200, 136], [1, 1, 1], 64)
    ref = reference_switch_off(wr, ch, 21)
    stays_call_by_call(wr, ch, on(wr, 21), ref)


def test_k_below_64_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 72, NS, [56, 200, 136], [1, 1, 1], 65)
    ref = reference_switch_off(wr, ch, 21)
    stays_call_by_call(wr, ch, on(wr, 21), ref)


def test_m_below_every_tile_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 24, NS, KS, [1, 1, 1], 66)
    ref = reference_switch_off(wr, ch, 20)
    stays_call_by_call(wr, ch, on(wr, 20), ref)


def test_an_n_below_every_tile_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 72, [200, 136, 56], KS, [1, 1, 1], 67)  # the last layer is 56 wide
    ref = reference_switch_off(wr, ch, 21)
    stays_call_by_call(wr, ch, on(wr, 21), ref)


def test_a_forced_generic_kernel_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 72, NS, KS, [1, 1, 1], 68)
    with b_image(wr, 2):
        wr.force_variant(8)
        try:
            ch.handles = [wr.fused_brgemm_dispatch(BF16, 72, NS[l], KS[l], ch.ld_in[l], ch.ldb[l], ch.ldc[l], KS[l], KS[l] * ch.ldb[l], ch.flags, 0, 5, 4, 1) for l in range(3)]
        finally:
            wr.force_variant(-1)
    ref = reference_switch_off(wr, ch, 21)
    stays_call_by_call(wr, ch, on(wr, 21), ref)


def test_synchronous_mode_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 72, NS, KS, [1, 1, 1], 69)
    ref = reference_switch_off(wr, ch, 21)
    try:
        stays_call_by_call(wr, ch, lambda: (on(wr, 21)(), wr.set_async(False)), ref)
    finally:
        wr.set_async(True)


def test_calls_that_differ_in_m_stay_call_by_call(wr):
    """the last call has 64 rows where the others have 72: it leaves rows 64 .. 71 of its output as they were"""
    ch = WidthsChain(wr, 2, 72, NS, KS, [1, 1, 1], 60, ms=[72, 72, 64])
    ref = reference_switch_off(wr, ch, 21)
    stays_call_by_call(wr, ch, on(wr, 21), ref, rows_=[72, 72, 64])


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_a_divisible_mixed_width_chain_is_the_chain_widths_switch_s(wr, t):
    bm, bn = TILE[t]
    ch = WidthsChain(wr, 2, 2 * bm, [3 * bn, bn, 2 * bn], [192, 3 * bn, bn], [1, 1, 1], 80 + t, tiles=t)
    seen = {}
    for new_sw, widths_sw in ((0, 0), (1, 0), (0, 1), (1, 1)):
        all_off(wr)
        wr.set_chain_widths_ragged(new_sw), wr.set_chain_widths(widths_sw)
        before, widths_before = wr.chain_widths_ragged_stats(), wr.chain_widths_stats()
        outs = ch.outputs()
        ran = wr.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        ch.check_windows(got)
        assert wr.chain_widths_ragged_stats() == before, "a chain the tile divides entirely moved the new mode's counter"
        assert ran == bool(widths_sw) and wr.chain_widths_stats()[0] == widths_before[0] + widths_sw
        seen[(new_sw, widths_sw)] = [digest(g) for g in got]
    assert len({tuple(v) for v in seen.values()}) == 1, seen


def test_a_ragged_width_equal_n_chain_is_the_chain_ragged_switch_s(wr):
    ch = RaggedChain(wr, 2, 72, 72, [200, 72, 72], [1, 1, 1], 90)
    seen = {}
    for sw in (0, 1):
        all_off(wr)
        wr.set_edge_tiles(21), wr.set_chain_ragged(1), wr.set_chain_widths_ragged(sw)
        before, ragged_before = wr.chain_widths_ragged_stats(), wr.chain_ragged_stats()
        outs = ch.outputs()
        ran = wr.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        ch.check_windows(got)
        assert ran and wr.chain_ragged_stats()[0] == ragged_before[0] + 1 and wr.chain_widths_ragged_stats() == before
        seen[sw] = [digest(g) for g in got]
    assert seen[0] == seen[1]


@pytest.mark.parametrize("t", [1, 3])
def test_a_ragged_m_equal_width_chain_is_the_chain_edge_switch_s(wr, t):
    bm, bn = TILE[t]
    ch = RaggedChain(wr, 2, 3 * bm - 3, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 95 + t)
    seen = {}
    for sw in (0, 1):
        all_off(wr)
        wr.set_edge_tiles(20 + t), wr.set_chain_edge(1), wr.set_chain_widths_ragged(sw)
        before, edge_before = wr.chain_widths_ragged_stats(), wr.chain_edge_stats()
        outs = ch.outputs()
        ran = wr.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        ch.check_windows(got)
        assert ran and wr.chain_edge_stats()[0] == edge_before[0] + 1 and wr.chain_widths_ragged_stats() == before
        seen[sw] = [digest(g) for g in got]
    assert seen[0] == seen[1]


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


@pytest.mark.parametrize("batch,layers,grid", [(200, [200, 136, 72, 200], (4, 4, 21)), (96, [784, 256, 128, 64], (2, 4, 21))])
def test_sharded_mlp_fuses_a_ragged_mixed_width_step_with_the_switch_on(wr, batch, layers, grid):
    """the 64x64 tile forced for the calls and for the launch (the tile decides the order of the sums: the 32x64 tile splits k over two wave
    groups), so the step has the same bits either way"""
    import torch
    spec = pkg.MlpSpec(batch=batch, layers=layers)
    X, Wv, Bs = mlp_problem(spec)
    seen = {}
    for sw in (0, 1):
        all_off(wr)
        singles(wr, 21), wr.set_chain_widths_ragged(sw)
        before = wr.chain_widths_ragged_stats()
        mlp = pkg.ShardedMlp(spec, 0, 1, wr)
        acts = [torch.full((spec.batch, n), float("nan"), dtype=torch.bfloat16, device="cuda") for n in spec.layers[1:]]
        mlp.forward(X, Wv, Bs, acts)
        wr.synchronize()
        assert bool(mlp.last_step_fused) == bool(sw), "switch %d" % sw
        assert wr.chain_widths_ragged_stats()[0] == before[0] + sw
        if sw:
            assert wr.chain_widths_ragged_stats()[1:] == grid
        assert not torch.isnan(acts[-1].float()).any() and acts[-1].float().abs().max() > 0
        seen[sw] = [digest(a.cpu().view(torch.int16).numpy()) for a in acts]
    assert seen[0] == seen[1], "the step as one launch and call by call differ"
