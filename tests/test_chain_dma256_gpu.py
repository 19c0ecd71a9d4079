"""Layer chains on the 256x256 bf16 tile (include/tpp_xsmm_abi.h xsmm_hip_set_chain_dma256) on a real MI355X: with the switch on, a bf16
chain whose m and n 256 divides runs as ONE launch of that tile's chain kernel (brgemm_bf16_dma256_chain.hip) - G x n / 256 resident
workgroups, each computing its tile of every layer and handing its rows over through a counter per row block.

Three layers with bias + relu, later layers k = n; B images VNNI-2, flat and VNNI-4. One round: 256 x 256 with k0 = 32 (one workgroup, a
self hand-off, one chunk in layer 0 and 8 behind it), 512 x 512 with k0 = 96 (2 x 2; 3 chunks then 16), 768 x 512 with k0 = 160 in two batch
elements (3 x 2, the linear map), 1024 x 512 with k0 = 224 (4 x 2, the XCD-blocked map). Rounds by forced G: 1280 x 256 on G = 2 (groups own
3 and 2 blocks), 1024 x 512 on G = 2, 768 x 256 on G = 1. Every buffer has 8 guard rows and 8 gap columns (tests/chain_edge_worker.py).
  1 exact inputs: every layer bit for bit the oracle's, one launch, the stats up by (+1, G, R, image), no other counter moves, guards intact
  2 random operands, six steps on NaN-refilled outputs with another layer-0 input every step: the bits of the same calls made one by one on
    the 256x256 tile with the switch off. (Every k0 above is 32 mod 64 and the library reaches the divisible kernel on k % 64 == 0 only:
    layer 0's separate call runs under xsmm_hip_set_dma256_edge(2) on m + 8 rows - unshifted whole tiles of the same kernel text over the
    chain's rows; the later layers are pinned by the forced variant / xsmm_hip_set_dma256_images(2).) Fails without the kernel.
  3 mode 1: calls forced onto the tile at dispatch (VNNI-2) or taken by xsmm_hip_set_dma256_images(2) are taken with the bits of the
    separate calls; the same shape planned by rule is not. A real overflow, VNNI-2, two layers, n = 256, m = 256 x (CUs + 8): R = 2 -
    under mode 1 with k0 = 64 (a call with k0 = 32 cannot be dispatched on the tile, which mode 1 asks of every call) and under mode 2
    with the issue's k0 = 32 on exact inputs, both against the separate calls on the GPU.
  4 as with the switch off - same bits, same return value, unmoved stats: mode 0, m = 384, n = 384, k0 = 40, an f32 chain, synchronous
    mode, layers of different n, a forced G > tiles_m
  5 strict mode (processes of their own): mode 1 on calls dispatched on the tile is one launch with the strict separate calls' bits; mode 2
    on other calls is refused
Every case resets the switch to 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chain_dma256_worker import KIND, V_DMA256, make_chain, separate_calls_on_the_tile
from chain_edge_worker import BF16, F32, RaggedChain, dev, digest
from oracle import pyoracle as orc
from test_chain_edge_gpu import check_exact

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m, n, k0, br0, mode) -> G, R
ONE_ROUND = [(256, 256, 32, 1, 2), (512, 512, 96, 1, 2), (768, 512, 160, 2, 2), (1024, 512, 224, 1, 2)]
ROUNDS = [(1280, 256, 32, 1, 1002), (1024, 512, 96, 1, 1002), (768, 256, 160, 1, 1001)]
SHAPES = ONE_ROUND + ROUNDS


def groups_rounds(m, mode):
    g = mode - 1000 if mode > 1000 else m // 256
    return g, -(-(m // 256) // g)


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture()
def sw(rt):
    """asynchronous mode for the case; whatever happens, the switch (and the two it is tested beside) is 0 afterwards"""
    was_async = rt.set_async(True)
    try:
        yield rt
    finally:
        rt.synchronize()
        rt.set_chain_dma256(0)
        rt.set_dma256_images(0)
        rt.set_dma256_edge(0)
        rt.force_variant(-1)
        rt.set_async(was_async)


def others(rt):
    return (rt.chain_edge_stats(), rt.chain_rounds_stats(), rt.chain_ragged_stats(), rt.chain_widths_stats(), rt.chain_width_rounds_stats(),
            rt.chain_widths_ragged_stats(), rt.dma256_edge_stats(), rt.dma256_images_stats(), rt.edge_tiles_stats())


def run_one_launch(rt, ch, mode, outs, dx=None, want=None):
    """the chain through xsmm_hip_fused_brgemm_chain_invoke under `mode`: one launch, counted as (+1, G, R, image), no other counter moves"""
    rt.set_chain_dma256(mode)
    before, o_before = rt.chain_dma256_stats(), others(rt)
    ran = rt.fused_brgemm_chain(BF16, ch.calls(outs, dx))
    rt.synchronize()
    after = rt.chain_dma256_stats()
    rt.set_chain_dma256(0)
    assert ran, "xsmm_hip_fused_brgemm_chain_invoke returned 0: the chain ran call by call"
    assert after == (before[0] + 1,) + (want or groups_rounds(ch.m, mode)) + (KIND[ch.image],), (before, after)
    assert others(rt) == o_before, "another chain / edge / dma256 counter moved"


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("m,n,k0,br0,mode", SHAPES)
def test_exact_inputs_one_launch_bit_for_bit_against_the_oracle(sw, m, n, k0, br0, mode, image):
    ch = make_chain(sw, image, m, n, k0, br0, m + n + k0 + image, exact=True)
    outs = ch.outputs()
    run_one_launch(sw, ch, mode, outs)
    got = ch.host(outs)
    ch.check_windows(got)
    check_exact(ch, got)


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("m,n,k0,br0,mode", SHAPES)
def test_random_operands_six_steps_have_the_bits_of_the_separate_calls_on_the_tile(sw, m, n, k0, br0, mode, image):
    ch = make_chain(sw, image, m, n, k0, br0, 7 * m + n + k0 + image, force=V_DMA256 if image == 2 else None)
    rng = np.random.default_rng(m + k0)
    outs = ch.outputs()
    for step in range(6):
        # another layer-0 input every step, into another buffer: a stale line of an earlier step's activations shows
        x = ch.x.copy().reshape(m + 8, -1)
        x[:m, :k0 * br0] = orc.f32_to_bf16(rng.uniform(-1, 1, m * k0 * br0).astype(np.float32)).reshape(m, -1)
        dx = dev(x.reshape(-1))
        want = separate_calls_on_the_tile(sw, ch, dx)
        ch.refill(outs)  # NaN inside, the sentinel around: a stale element of an earlier step cannot pass
        run_one_launch(sw, ch, mode, outs, dx)
        got = ch.host(outs)
        ch.check_windows(got)
        for l in range(ch.L):
            assert np.array_equal(got[l], want[l]), "step %d layer %d: %d elements differ from the separate calls" % (step, l, int((got[l] != want[l]).sum()))
        if step:
            assert not np.array_equal(want[-1], last), "the steps' inputs did not differ"
        last = want[-1]
    assert np.abs(orc.bf16_to_f32(want[-1].reshape(m + 8, -1)[:m, :n].copy().reshape(-1))).max() > 0


@pytest.mark.parametrize("image", [2, 0, 4])
def test_mode_1_takes_calls_that_run_on_the_tile_and_no_others(sw, image):
    m, n = 1024, 512
    on = make_chain(sw, image, m, n, 512, 1, 300 + image, force=V_DMA256 if image == 2 else None)
    want = separate_calls_on_the_tile(sw, on)
    if image != 2:
        sw.set_dma256_images(2)  # (what takes a flat / VNNI-4 call onto the tile, and what mode 1 reads)
    outs = on.outputs()
    run_one_launch(sw, on, 1, outs)
    got = on.host(outs)
    on.check_windows(got)
    for l in range(on.L):
        assert np.array_equal(got[l], want[l]), "layer %d" % l
    # the same shape planned by rule goes elsewhere (8 tiles of 256x256): not taken, everything as with the switch off
    sw.set_dma256_images(0)
    off = make_chain(sw, image, m, n, 512, 1, 300 + image)
    seen = {}
    for mode in (0, 1):
        sw.set_chain_dma256(mode)
        before = sw.chain_dma256_stats()
        outs = off.outputs()
        ran = sw.fused_brgemm_chain(BF16, off.calls(outs))
        got = off.host(outs)
        off.check_windows(got)
        assert sw.chain_dma256_stats() == before
        seen[mode] = (ran, [digest(g) for g in got])
    assert seen[1] == seen[0], seen


@pytest.mark.parametrize("mode,k0", [(1, 64), (2, 32)])
def test_a_real_overflow_runs_in_two_rounds(sw, mode, k0):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = 256 * (cus + 8)
    ch = make_chain(sw, 2, m, 256, k0, 1, 41 + k0, layers=2, exact=mode == 2, force=V_DMA256)
    sw.set_chain_dma256(0)
    outs = ch.outputs()
    ch.one_by_one(outs)  # (mode 1: both calls on the tile; mode 2: exact inputs, every kernel has the oracle's bits)
    want = ch.host(outs)
    outs = ch.outputs()
    run_one_launch(sw, ch, mode, outs, want=(-(-(cus + 8) // 2), 2))  # Gmax = CUs: R = 2, G = ceil((CUs + 8) / 2)
    got = ch.host(outs)
    ch.check_windows(got)
    for l in range(ch.L):
        assert np.array_equal(got[l], want[l]), "layer %d: %d elements differ" % (l, int((got[l] != want[l]).sum()))


def as_with_the_switch_off(rt, ch, mode, settings=lambda: None):
    """under `mode` the chain invoke returns what it returns with the switch off, has those bits and moves no counter of this switch"""
    seen = {}
    for md in (0, mode):
        settings()
        rt.set_chain_dma256(md)
        before = rt.chain_dma256_stats()
        outs = ch.outputs()
        ran = rt.fused_brgemm_chain(ch.dtype, ch.calls(outs))
        got = ch.host(outs)
        rt.set_chain_dma256(0)
        ch.check_windows(got)
        assert rt.chain_dma256_stats() == before, "the counter moved"
        seen[md] = (bool(ran), [digest(g) for g in got])
    assert seen[mode] == seen[0], seen
    return seen[0][0]


def test_mode_0_and_shapes_the_tile_does_not_divide_are_as_with_the_switch_off(sw):
    as_with_the_switch_off(sw, make_chain(sw, 2, 512, 512, 96, 1, 50), 0)
    as_with_the_switch_off(sw, make_chain(sw, 2, 384, 256, 96, 1, 51), 2)       # m = 384
    as_with_the_switch_off(sw, make_chain(sw, 2, 512, 384, 96, 1, 52), 2)       # n = 384
    as_with_the_switch_off(sw, make_chain(sw, 2, 512, 512, 40, 1, 53), 2)       # k0 = 40
    as_with_the_switch_off(sw, make_chain(sw, 2, 768, 256, 160, 1, 54), 1004)   # a forced G > tiles_m


def test_an_f32_chain_is_as_with_the_switch_off(sw):
    as_with_the_switch_off(sw, RaggedChain(sw, 0, 512, 256, [64, 256, 256], [1, 1, 1], 55, dtype=F32), 2)


def test_synchronous_mode_is_as_with_the_switch_off(sw):
    ch = make_chain(sw, 2, 512, 512, 96, 1, 56)
    try:
        assert as_with_the_switch_off(sw, ch, 2, lambda: sw.set_async(False)) is False
    finally:
        sw.set_async(True)


def test_layers_of_different_n_are_as_with_the_switch_off(sw):
    """512 rows: 256 columns in layer 0, 512 in the two behind it (layer 1 reads the 256 columns of layer 0's rows: its lda is a.ldc)"""
    m = 512
    a, b = make_chain(sw, 2, m, 256, 96, 1, 57, layers=1), make_chain(sw, 2, m, 512, 256, 1, 58, layers=2)
    assert b.ld_in[0] == a.ldc
    seen = {}
    for md in (0, 2):
        sw.set_chain_dma256(md)
        before = sw.chain_dma256_stats()
        oa, ob = a.outputs(), b.outputs()
        calls = a.calls(oa) + b.calls(ob, oa[0])
        ran = sw.fused_brgemm_chain(BF16, calls)
        got = a.host(oa) + b.host(ob)
        sw.set_chain_dma256(0)
        assert sw.chain_dma256_stats() == before
        seen[md] = (bool(ran), [digest(g) for g in got])
    assert seen[2] == seen[0], seen


def worker(image, m, n, k0, br0, force, seed, mode):
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_STRICT", "TPP_HIP_CHAIN_DMA256", "TPP_HIP_CHAIN", "TPP_HIP_VNNI_FACTOR")}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_CHAIN_DMA256=str(mode))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_dma256_worker.py")] + [str(x) for x in (image, m, n, k0, br0, force, seed)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["mode_from_env"] == mode, d
    return d


def test_strict_mode_takes_calls_dispatched_on_the_tile_and_refuses_others():
    # mode 1, every call forced onto the tile at dispatch: one launch, the bits of the strict separate calls
    on, ref = worker(2, 1024, 512, 512, 1, V_DMA256, 71, 1), worker(2, 1024, 512, 512, 1, V_DMA256, 71, 0)
    assert on["ran_as_one"] is True and on["chain_dma256_stats"] == [1, 4, 1, 0], on
    assert ref["chain_dma256_stats"][0] == 0 and on["digests"] == ref["digests"]
    # mode 2 on calls planned elsewhere: refused - everything as with the switch off
    other, ref = worker(2, 1024, 512, 512, 1, -1, 72, 2), worker(2, 1024, 512, 512, 1, -1, 72, 0)
    assert other["chain_dma256_stats"][0] == 0 and other["ran_as_one"] == ref["ran_as_one"] and other["digests"] == ref["digests"], (other, ref)
