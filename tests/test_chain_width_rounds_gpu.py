"""Column rounds of mixed-width bf16 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_width_rounds) on a real MI355X: with the switch on,
a bf16 chain whose layers differ in n runs as ONE launch of the chain kernel (brgemm_bf16_lw GRP = 10, brgemm_bf16_lw_chain_wrounds.hip) on
m / BM x W workgroups, W below the widest layer's column tiles; workgroup (tm, c) walks the column tiles c, c + W, .. of every layer that
has them and sits out the others (brgemm_bf16_lw_chain_wrounds.h).

Buffers as in chain_widths_worker.WidthsChain: 8 guard rows and 8 gap columns around everything, NaN around the inputs, a sentinel around
the outputs, checked after every run. For tile t = 0 .. 3 - (BM, BN) = (32, 64), (64, 64), (64, 128), (128, 128) - and the B images VNNI-2,
flat and VNNI-4, all calls dispatched under force_variant(BASE[image] + t) so that the launch and the separate calls share the tile;
m = 2 BM unless said; layer 0 takes k = 192 unless said; W forced with 1000 + W. Width vectors and W:
  [4 BN, BN, 2 BN]  W = 2     two rounds, then a column group that sits out a layer and resumes
  [4 BN, BN, 2 BN]  W = 3     unequal step counts per group
  [BN, 3 BN, BN]    W = 1     every layer a walk of T_l steps on one workgroup column
  [2 BN, BN] * 4    W = 1     eight layers
  [2 BN, 2 BN, BN]  W = 1     two batch elements per layer
  [3 BN, BN]        W = 2     three batch elements of k = 256 in layer 0: 12 chunks, more than any ring
  [4 BN, 2 BN]      W = 2     m = 3 BM
  [1024, 512, 1024] W = 3     k0 = 512: every layer has at least a ring of chunks - the B loaders run ahead into every next step
  1 exact inputs, bias + relu: every layer bit for bit the oracle's, one launch, this mode's counter up by one with (m / BM, W, variant),
    no other chain or single-call counter moved, guard windows intact
  2 random operands, six steps on refilled outputs: exact equality with the same calls made one by one with every switch off
  3 two chains with one grid and different inner widths alternate three times each on one stream
  4 the rule (mode 1) on 1024 rows x [640, 64, 640] dispatched on the 32x64 tile - 32 x 10 tiles, more than the compute units: one
    launch with the header's balanced W, the bits of the separate calls; with set_chain_widths(1) alone the same chain returns 0
  5 call by call with the switch-off bits: the switch off, f32, a ragged m under set_chain_edge(1), an n_l no tile divides, k = 200 under
    set_chain_ragged(1), synchronous mode, 1000 + W with W >= max T, 1000 + W with m / BM * W above the compute units, strict mode with
    calls dispatched on different tiles (a process of its own)
  6 with the switch at 1 an equal-width chain runs the plain chain kernel and, under set_chain_widths(1), a funnel that fits runs the
    one-round mixed-width launch: the same digests as with the switch at 0, this mode's counter unmoved
  7 ShardedMlp(MlpSpec(batch=256, layers=[256, 512, 128, 256])) under force_variant(21) and mode 1002
No test tries to provoke a starved or timed-out launch. Every case leaves every switch at 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chain_edge_worker import BASE, BF16, F32, TILE, digest
from chain_width_rounds_worker import balanced_w
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
    rt.set_chain_width_rounds(0), rt.set_chain_widths(0), rt.set_chain_ragged(0), rt.set_chain_edge(0), rt.set_chain_rounds(0)
    rt.set_edge_tiles(0), rt.set_edge_k_bf16(0), rt.set_edge_k8_bf16(0)
    rt.force_variant(-1)


@pytest.fixture()
def wr(rt):
    """asynchronous mode for the case; whatever happens, every switch - this one too - is 0 afterwards"""
    was_async = rt.set_async(True)
    all_off(rt)
    try:
        yield rt
    finally:
        rt.synchronize()
        all_off(rt)
        rt.set_async(was_async)


def other_counters(rt):
    return (rt.chain_widths_stats(), rt.chain_edge_stats(), rt.chain_rounds_stats(), rt.chain_ragged_stats(), rt.edge_tiles_stats(), rt.edge_k_bf16_stats(),
            rt.edge_k8_bf16_stats())


def chain_counters(rt):
    return (rt.chain_width_rounds_stats(), rt.chain_widths_stats(), rt.chain_edge_stats(), rt.chain_rounds_stats(), rt.chain_ragged_stats())


def run_one_launch(rt, ch, t, w, outs, mode=None):
    """the chain through xsmm_hip_fused_brgemm_chain_invoke with the switch on (1000 + w unless `mode`): one launch, counted, nothing else counted"""
    bm, _ = TILE[t]
    all_off(rt)
    rt.set_chain_width_rounds(1000 + w if mode is None else mode)
    before, others = rt.chain_width_rounds_stats(), other_counters(rt)
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    rt.synchronize()
    after = rt.chain_width_rounds_stats()
    rt.set_chain_width_rounds(0)
    assert ran, "xsmm_hip_fused_brgemm_chain_invoke returned 0: the chain ran call by call"
    assert after == (before[0] + 1, ch.m // bm, w, BASE[ch.image] + t), (before, after)
    assert other_counters(rt) == others, "another chain or single-call counter moved"


def separate_calls(rt, ch):
    """the same calls one by one (dispatched on the same tile) with every switch off"""
    all_off(rt)
    outs = ch.outputs()
    before = chain_counters(rt)
    ch.one_by_one(outs)
    got = ch.host(outs)
    assert chain_counters(rt) == before
    return got


def specs(t):
    """(rows in row blocks, ns, ks, brs, W) of tile t's chains"""
    bn = TILE[t][1]
    chain = lambda ns, w, k0=192, mb=2: (mb, ns, [k0] + ns[:-1], [1] * len(ns), w)
    return [chain([4 * bn, bn, 2 * bn], 2), chain([4 * bn, bn, 2 * bn], 3), chain([bn, 3 * bn, bn], 1), chain([2 * bn, bn] * 4, 1),
            (2, [2 * bn, 2 * bn, bn], [192, bn, bn], [2, 2, 2], 1),
            (2, [3 * bn, bn], [256, 3 * bn], [3, 1], 2),
            chain([4 * bn, 2 * bn], 2, mb=3),
            chain([1024, 512, 1024], 3, k0=512)]


def chains(rt, t, image, seed, exact):
    return [(WidthsChain(rt, image, mb * TILE[t][0], ns, ks, brs, seed + i, exact=exact, tiles=t), w) for i, (mb, ns, ks, brs, w) in enumerate(specs(t))]


def takes(ch):
    """does the chain pass the conditions this mode shares with xsmm_hip_set_chain_widths? One of the vectors does not, on one tile with one
    image: the VNNI-2 image of the loader-wave tiles asks for m % 64 == 0 (gemm_plan.cpp bf16_lw_b_kind), and m = 3 BM is 96 on the 32x64
    tile. There the chain stays call by call, with the bits of the separate calls - checked in its place."""
    return not (ch.image == 2 and ch.m % 64)


def one_launch_or_call_by_call(rt, ch, t, w, outs):
    if takes(ch):
        run_one_launch(rt, ch, t, w, outs)
        return
    all_off(rt)
    rt.set_chain_width_rounds(1000 + w)
    before = chain_counters(rt)
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    rt.synchronize()
    rt.set_chain_width_rounds(0)
    assert not ran and chain_counters(rt) == before


def test_the_width_vectors_cover_the_schedule_s_cases():
    ring = [8, 8, 6, 4]  # BLW_TILES[t].nslot
    for t in range(4):
        bn = TILE[t][1]
        sp = specs(t)
        assert all(n % bn == 0 for _, ns, _, _, _ in sp for n in ns)
        tiles = [([n // bn for n in ns], w) for _, ns, _, _, w in sp]
        assert all(1 <= w < max(v) for v, w in tiles), "fewer workgroup columns than the widest layer has column tiles"
        assert any(max(v) == 2 * w and any(a > b < c and b < w for a, b, c in zip(v, v[1:], v[2:])) for v, w in tiles), "two rounds, a group sits out a layer and resumes"
        assert any(len({len(range(c, max(v), w)) for c in range(w)}) > 1 for v, w in tiles), "unequal step counts per group"
        assert any(w == 1 and v[0] < max(v) for v, w in tiles), "every layer a walk on one workgroup column"
        assert any(len(v) == 8 for v, _ in tiles)
        assert any(all(b == 2 for b in brs) for _, _, _, brs, _ in sp)
        chunks = [[b * (k // 64) for k, b in zip(ks, brs)] for _, _, ks, brs, _ in sp]
        assert any(cs[0] == 12 for cs in chunks), "more chunks than any ring"
        assert any(mb == 3 for mb, _, _, _, _ in sp)
        for image in (2, 0, 4):  # m = 3 BM runs as one launch everywhere but on 32x64 with VNNI-2 (takes)
            assert [mb for mb, _, _, _, _ in sp if image == 2 and (mb * TILE[t][0]) % 64] == ([3] if (t, image) == (0, 2) else [])
        assert any(all(c >= ring[t] for c in cs) for cs in chunks), "the B loaders' run-ahead"
        assert any(any(c < ring[t] for c in cs) for cs in chunks), "... and no run-ahead"


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_one_launch_bit_for_bit_against_the_oracle(wr, t, image):
    for ch, w in chains(wr, t, image, 1000 * t + 100 * image, exact=True):
        outs = ch.outputs()
        one_launch_or_call_by_call(wr, ch, t, w, outs)
        got = ch.host(outs)
        ch.check_windows(got)
        check_exact(ch, got)


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_six_steps_have_the_bits_of_the_separate_calls(wr, t, image):
    for ch, w in chains(wr, t, image, 5000 + 1000 * t + 100 * image, exact=False):
        want = separate_calls(wr, ch)
        outs = ch.outputs()
        for step in range(6):
            ch.refill(outs)  # NaN inside, the sentinel around: a stale element of an earlier step cannot pass
            one_launch_or_call_by_call(wr, ch, t, w, outs)
            got = ch.host(outs)
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[l]), "m %d ns %s W %d step %d layer %d: %d elements differ from the separate calls" % (
                    ch.m, ch.ns, w, step, l, int((got[l] != want[l]).sum()))
        assert (want[-1].reshape(ch.m + 8, -1)[:ch.m, :ch.ns[-1]] & 0x7fff).max() > 0


@pytest.mark.parametrize("t,image", [(0, 2), (1, 0), (2, 4), (3, 2)])
def test_two_chains_with_one_grid_and_different_inner_widths_alternate_on_one_stream(wr, t, image):
    bm, bn = TILE[t]
    a = WidthsChain(wr, image, 2 * bm, [4 * bn, bn, 4 * bn], [192, 4 * bn, bn], [1, 1, 1], 300 + t, tiles=t)
    b = WidthsChain(wr, image, 2 * bm, [bn, 4 * bn, 4 * bn], [192, bn, 4 * bn], [1, 1, 1], 310 + t, tiles=t)
    want = {id(ch): separate_calls(wr, ch) for ch in (a, b)}
    outs = {id(ch): ch.outputs() for ch in (a, b)}
    for step in range(3):
        for ch in (a, b):
            ch.refill(outs[id(ch)])
            run_one_launch(wr, ch, t, 2, outs[id(ch)])
            got = ch.host(outs[id(ch)])
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], want[id(ch)][l]), "ns %s step %d layer %d" % (ch.ns, step, l)


def stream_cus():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def wide_chain(rt, seed):
    """1024 rows x [640, 64, 640] on the 32x64 tile: 32 x 10 output tiles in the wide layers"""
    return WidthsChain(rt, 2, 1024, [640, 64, 640], [64, 640, 64], [1, 1, 1], seed, tiles=0)


def test_the_rule_takes_a_chain_whose_widest_layer_exceeds_the_compute_units(wr):
    cus = stream_cus()
    assert 32 * 10 > cus >= 32, "the case is written for a device with 32 .. 319 compute units"
    ch = wide_chain(wr, 400)
    want = separate_calls(wr, ch)
    # the one-round rule refuses it: more tiles than compute units
    all_off(wr)
    wr.set_chain_widths(1)
    before = chain_counters(wr)
    outs = ch.outputs()
    assert not wr.fused_brgemm_chain(BF16, ch.calls(outs))
    got = ch.host(outs)
    assert chain_counters(wr) == before
    for l in range(ch.L):
        assert np.array_equal(got[l], want[l])
    # ... this one takes it, on the header's balanced W, with the bits of the separate calls
    w = balanced_w(10, 32, cus)
    assert 1 <= w < 10
    ch.refill(outs)
    run_one_launch(wr, ch, 0, w, outs, mode=1)
    got = ch.host(outs)
    ch.check_windows(got)
    for l in range(ch.L):
        assert np.array_equal(got[l], want[l]), "layer %d" % l


def stays_call_by_call(rt, ch, settings, reference, rows=None):
    """under `settings` the chain invoke returns 0 and moves no chain counter; its bits are those of `reference`"""
    all_off(rt)
    settings()
    before = chain_counters(rt)
    outs = ch.outputs()
    ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
    got = ch.host(outs)
    rt.set_chain_width_rounds(0)
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


def test_the_switch_off_stays_call_by_call_and_the_same_chain_is_taken_with_it_on(wr):
    ch = WidthsChain(wr, 2, 128, [256, 64, 128], [192, 256, 64], [1, 1, 1], 61, tiles=1)
    ref = reference_switch_off(wr, ch)
    stays_call_by_call(wr, ch, lambda: None, ref)
    outs = ch.outputs()
    run_one_launch(wr, ch, 1, 2, outs, mode=1)  # (max T = 4 fits in one round: the rule makes two balanced rounds of it)
    got = ch.host(outs)
    for l in range(ch.L):
        assert np.array_equal(got[l], ref[l])


@pytest.mark.parametrize("mode", [1, 1002])
def test_an_f32_chain_stays_call_by_call(wr, mode):
    ch = WidthsChain(wr, 0, 128, [256, 64, 128], [192, 256, 64], [1, 1, 1], 62, dtype=F32)
    ref = reference_switch_off(wr, ch)
    stays_call_by_call(wr, ch, lambda: wr.set_chain_width_rounds(mode), ref)


@pytest.mark.parametrize("mode", [1, 1002])
def test_a_ragged_m_stays_call_by_call_under_the_chain_edge_switch(wr, mode):
    ch = WidthsChain(wr, 2, 125, [256, 64, 128], [192, 256, 64], [1, 1, 1], 64)
    ref = reference_switch_off(wr, ch, lambda: wr.set_edge_tiles(21))
    stays_call_by_call(wr, ch, lambda: (wr.set_edge_tiles(21), wr.set_chain_edge(1), wr.set_chain_width_rounds(mode)), ref)


@pytest.mark.parametrize("mode", [1, 1001])
def test_an_n_no_tile_divides_stays_call_by_call(wr, mode):
    """n_1 = 96: 96 % 64 != 0 and 96 % 128 != 0 (layer 2 reads its first 64 columns)"""
    ch = WidthsChain(wr, 2, 128, [128, 96, 128], [192, 128, 64], [1, 1, 1], 65)
    ref = reference_switch_off(wr, ch, lambda: wr.set_edge_tiles(21))
    stays_call_by_call(wr, ch, lambda: (wr.set_edge_tiles(21), wr.set_chain_ragged(1), wr.set_chain_width_rounds(mode)), ref)


@pytest.mark.parametrize("mode", [1, 1001])
def test_a_k_of_200_stays_call_by_call_under_the_chain_ragged_switch(wr, mode):
    ch = WidthsChain(wr, 2, 128, [128, 64, 128], [200, 128, 64], [1, 1, 1], 66)
    singles = lambda: (wr.set_edge_tiles(21), wr.set_edge_k_bf16(21), wr.set_edge_k8_bf16(21))
    ref = reference_switch_off(wr, ch, singles)
    stays_call_by_call(wr, ch, lambda: (singles(), wr.set_chain_ragged(1), wr.set_chain_width_rounds(mode)), ref)


def test_synchronous_mode_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 128, [256, 64, 128], [192, 256, 64], [1, 1, 1], 67, tiles=1)
    ref = reference_switch_off(wr, ch)
    try:
        stays_call_by_call(wr, ch, lambda: (wr.set_chain_width_rounds(1), wr.set_async(False)), ref)
    finally:
        wr.set_async(True)


def test_a_forced_w_of_the_widest_layer_s_column_tiles_or_more_stays_call_by_call(wr):
    ch = WidthsChain(wr, 2, 128, [256, 64, 128], [192, 256, 64], [1, 1, 1], 69, tiles=1)
    ref = reference_switch_off(wr, ch)
    for w in (4, 5, 64):
        stays_call_by_call(wr, ch, lambda: wr.set_chain_width_rounds(1000 + w), ref)


def test_a_forced_w_above_the_compute_units_stays_call_by_call(wr):
    cus = stream_cus()
    w = cus // 32 + 1
    assert w < 10, "the case is written for a device with fewer than 288 compute units"
    ch = wide_chain(wr, 401)
    ref = reference_switch_off(wr, ch)
    stays_call_by_call(wr, ch, lambda: wr.set_chain_width_rounds(1000 + w), ref)


def test_strict_mode_with_calls_dispatched_on_different_tiles_stays_call_by_call(wr):
    image, m, seed, ns, tiles = 2, 128, 68, [256, 128, 256], [1, 2, 1]
    ch = WidthsChain(wr, image, m, ns, [192] + ns[:-1], [1, 1, 1], seed, tiles=tiles)
    want = separate_calls(wr, ch)
    all_off(wr)
    # strict mode is chosen before anything is queued: a fresh child process (the switch arrives through the environment there)
    drop = ("TPP_HIP_STRICT", "TPP_HIP_EDGE_TILES", "TPP_HIP_EDGE_K_BF16", "TPP_HIP_EDGE_K8_BF16", "TPP_HIP_CHAIN_EDGE", "TPP_HIP_CHAIN_RAGGED", "TPP_HIP_CHAIN_ROUNDS",
            "TPP_HIP_CHAIN_WIDTHS", "TPP_HIP_CHAIN_WIDTH_ROUNDS", "TPP_HIP_CHAIN", "TPP_HIP_VNNI_FACTOR")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_CHAIN_WIDTH_ROUNDS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_width_rounds_worker.py"), str(image), str(m), str(seed), ",".join(map(str, ns)), ",".join(map(str, tiles))],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["chain_width_rounds_from_env"] == 1
    assert d["ran_as_one"] is False and d["chain_width_rounds_stats"][0] == 0 and d["chain_widths_stats"][0] == 0
    assert d["digests"] == [digest(w) for w in want], "strict mode runs the calls one by one on their own tiles: the same bits"


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_an_equal_width_chain_and_a_funnel_of_the_one_round_rule_run_as_before(wr, t):
    bm, bn = TILE[t]
    equal = WidthsChain(wr, 2, 2 * bm, [2 * bn] * 3, [192, 2 * bn, 2 * bn], [1, 1, 1], 80 + t, tiles=t)
    funnel = WidthsChain(wr, 2, 2 * bm, [4 * bn, 2 * bn, bn], [192, 4 * bn, 2 * bn], [1, 1, 1], 90 + t, tiles=t)
    for ch, widths in ((equal, 0), (funnel, 1)):
        seen = {}
        for sw in (0, 1):
            all_off(wr)
            wr.set_chain_widths(widths), wr.set_chain_width_rounds(sw)
            mine, one_round = wr.chain_width_rounds_stats(), wr.chain_widths_stats()
            outs = ch.outputs()
            ran = wr.fused_brgemm_chain(BF16, ch.calls(outs))
            got = ch.host(outs)
            wr.set_chain_width_rounds(0)
            ch.check_windows(got)
            assert wr.chain_width_rounds_stats() == mine, "this mode's counter moved"
            assert wr.chain_widths_stats()[0] == one_round[0] + widths, "the funnel runs the one-round mixed-width launch, the equal-width chain the plain one"
            seen[sw] = (bool(ran), [digest(g) for g in got])
        assert seen[0][0] is True and seen[1] == seen[0], seen


def test_sharded_mlp_fuses_a_mixed_width_step_in_two_column_groups(wr):
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
    for sw in (0, 1002):
        all_off(wr)
        wr.set_chain_width_rounds(sw)
        before = wr.chain_width_rounds_stats()
        wr.force_variant(21)
        try:
            mlp = pkg.ShardedMlp(spec, 0, 1, wr)
            acts = [torch.full((spec.batch, n), float("nan"), dtype=torch.bfloat16, device="cuda") for n in spec.layers[1:]]
            mlp.forward(X, Wv, Bs, acts)
        finally:
            wr.force_variant(-1)
        wr.synchronize()
        wr.set_chain_width_rounds(0)
        assert bool(mlp.last_step_fused) == bool(sw), "switch %d" % sw
        assert wr.chain_width_rounds_stats()[0] == before[0] + (1 if sw else 0)
        if sw:
            assert wr.chain_width_rounds_stats()[1:] == (4, 2, 21)
        assert not torch.isnan(acts[-1].float()).any() and acts[-1].float().abs().max() > 0
        seen[sw] = [digest(a.cpu().view(torch.int16).numpy()) for a in acts]
    assert seen[0] == seen[1002], "the step as one launch and call by call differ"
