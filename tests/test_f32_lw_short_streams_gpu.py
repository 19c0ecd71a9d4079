"""Short chunk streams and seams on the f32 loader-wave tiles, on a real MI355X. The MFMA waves compute where their fragments lie in the
ring, where they park and what they store ABOVE the "chunk 0 published" barrier, and a loader wave finishes its setup behind its first
request (brgemm_f32_lw_tile.h mfma_setup, tail_setup, Loader::issue_first). What can go wrong with that is a stream shorter than the
ring, a ring lap that ends early, and the seam between two layers of a chain - so every tile runs
  T = 1, 2, 3, 4, 5 and 7 chunks (k = 64, br = T) and T = 2 as one batch element of k = 128,
on one to four tiles of output, beta 0 and beta 1, with and without bias + relu, and with padded lda / ldb / ldc, operand offsets and
poisoned memory around every operand and the output:
  1 exact inputs (tests/exact_data.py), bit for bit against the oracle, nothing written outside the window: the 64x64 + K2 tile as it
    has always been launched (halves off), the same call as halves, 64x32 + K4, 32x32 + K4 - with the batch-reduce split off (the plain
    instance) and, from two chunks on, forced to two workgroups per tile (the split instance)
  2 the halves against the plain launch on N(0, 1) operands, bit for bit (tests/test_f32_halves_gpu.py Layer.both)
  3 two and three f32 layers of 64-row batches through xsmm_hip_fused_brgemm_chain_invoke on both chain tiles, bit for bit against the
    same calls one by one, at one, two, three and five chunks per layer
Every case puts the switches back."""
import importlib

import numpy as np
import pytest

import exact_data as ed
from test_chain_f32_gpu import Chain32
from test_f32_halves_gpu import Layer
from test_parity_gpu import F32, dev, gemm_case

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")

# forced variant -> (the kernel name of the handle, the output sizes: one workgroup's worth up to four tiles)
TILES = {6: ("64x64,k2", (64, 128)), 7: ("64x32,k4", (64, 128)), 9: ("32x32,k4", (32, 64))}
# (k, br): T = 1, 2, 3, 4, 5, 7 chunks of one batch element each, and T = 2 inside one batch element
STREAMS = [(64, 1), (64, 2), (64, 3), (64, 4), (64, 5), (64, 7), (128, 1)]
EPILOGUES = [dict(beta0=True), dict(), dict(beta0=True, bias=True, relu=True), dict(bias=True, relu=True),
             dict(bias=True, relu=True, padded=True), dict(beta0=True, padded=True)]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def exact_cases(rt, variant, k, br, halves, split, seed):
    """every output size of the tile x every epilogue, exact inputs against the oracle; returns the refined kernels seen"""
    name, sizes = TILES[variant]
    K = k * br
    seen = set()
    prev_halves, prev_split = rt.set_f32_halves(halves), rt.force_split(split)
    assert prev_halves >= 0
    try:
        for m in sizes:
            for n in sizes:
                for i, ep in enumerate(EPILOGUES):
                    kw = dict(ep)
                    if kw.pop("padded", False):  # rows longer than they hold, operands at offsets, everything not named poisoned
                        kw.update(lda=K + 8, ldb=n + 4, ldc=n + 12, sb=k * (n + 4), offs=(4, 8, 4, 4), poison=True)
                    else:
                        kw.update(lda=K, ldb=n, sb=k * n)
                    before = rt.f32_halves_stats()
                    gemm_case(rt, F32, m, n, k, br, sa=k, values="exact", ranges=ed.exact_ranges(F32, K), seed=seed + 7 * i + m + 2 * n,
                              force=variant, expect=name, **kw)
                    moved = rt.f32_halves_stats()[0] - before[0]
                    assert moved == (1 if halves == 2 else 0), (variant, m, n, k, br, ep, moved)
                    seen.add(rt.last_refined_kernel())
    finally:
        rt.force_split(prev_split)
        rt.set_f32_halves(prev_halves)
    return seen


@pytest.mark.parametrize("k,br", STREAMS)
@pytest.mark.parametrize("variant", sorted(TILES))
def test_plain_instances_exact_against_the_oracle(rt, variant, k, br):
    """halves off, split off: brgemm_f32_lw<tile> as the handle names it"""
    assert exact_cases(rt, variant, k, br, 0, 1, 100 * variant + k + br) == {""}


@pytest.mark.parametrize("k,br", STREAMS)
def test_halves_exact_against_the_oracle(rt, k, br):
    """the 64x64 + K2 call as two 64x32 + K2 workgroups per tile, on their 3-slot ring (m, n in whole 64x64 tiles)"""
    assert exact_cases(rt, 6, k, br, 2, 1, 1000 + k + br) == {""}


@pytest.mark.parametrize("k,br", [s for s in STREAMS if s[0] * s[1] > 64])
@pytest.mark.parametrize("variant", sorted(TILES))
def test_split_instances_exact_against_the_oracle(rt, variant, k, br):
    """two workgroups per output tile: each runs its half of the chunk stream (T = 1 .. 4, the second one not from chunk 0)"""
    seen = exact_cases(rt, variant, k, br, 0, 2, 2000 + 100 * variant + k + br)
    assert all(s.endswith(", split") for s in seen), seen


@pytest.mark.parametrize("k,br", STREAMS)
def test_halves_have_the_bits_of_the_plain_launch(rt, k, br):
    """N(0, 1) operands: any change in the order of additions shows. Mode 0 against mode 2, window, row padding and guard band"""
    seed = 3000 + k + br
    for m, n in ((64, 64), (128, 128)):
        Layer(rt, m, n, k, br, seed=seed).both()
        Layer(rt, m, n, k, br, beta0=False, seed=seed + 1).both()
        Layer(rt, m, n, k, br, bias=True, relu=True, seed=seed + 2).both()
        Layer(rt, m, n, k, br, beta0=False, bias=True, relu=True, pad=True, seed=seed + 3).both()


@pytest.mark.parametrize("chunks", [1, 2, 3, 5])
@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("variant", [6, 7])
def test_chain_seams_have_the_bits_of_the_calls_one_by_one(rt, variant, layers, chunks):
    """64-row batches, every layer `chunks` chunks long (width 64 * chunks): the setup is redone at every seam, the ring restarts at
    slot 0. Two steps on the same buffers: a stale read at the seam would show the first step's values"""
    import torch
    width = 64 * chunks
    ch = Chain32(rt, 64, [width] * (layers + 1), seed=10 * variant + layers + chunks, force=variant)
    start = [np.full(ch.m * ch.ld[l + 1], np.nan, np.float32) for l in range(ch.L)]  # NaN: an unwritten element cannot pass
    dacts_f, dacts_s = [dev(a) for a in start], [dev(a) for a in start]
    was_async = rt.set_async(True)
    try:
        for step in range(2):
            dx = dev(ch.new_input())
            fused = rt.fused_brgemm_chain(F32, ch.calls(dx, dacts_f))
            for c in ch.calls(dx, dacts_s):
                rt.fused_brgemm(F32, *c)
            rt.synchronize()
            assert fused, "the chain did not run as one launch"
            for l in range(ch.L):
                assert torch.equal(dacts_f[l].view(torch.int32), dacts_s[l].view(torch.int32)), "step %d layer %d" % (step, l)
                assert not torch.isnan(dacts_f[l]).any()
    finally:
        rt.synchronize()
        rt.set_async(was_async)
