"""The GEMM case lists of the parity suite again, with POISONED surroundings (gemm_case(poison=True), tests/exact_data.py): every
element the descriptor does not name - lda / ldb padding (VNNI-2 / VNNI-4 layouts included), gaps between batch elements, guard tails
of A, B and the bias, the whole C window under beta = 0 - is NaN (f32: NaN, +inf, -inf). A kernel that zero-pads one operand at an
edge but reads the other's real memory there computes 0 * NaN and fails; the oracle runs on the same buffers and stays finite, which
proves the live mask covers everything it reads. Buffers keep their guard space: an over-read sees wrong values, not a fault."""
import importlib

import numpy as np
import pytest

import exact_data as ed
from oracle import pyoracle as orc
from test_parity_gpu import (BF16, BF16_CASES, BF16_FORCED, BF16_SMALL, F32, F32_FAST, RAGGED, dev, gemm_case,
                             host)

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def _id(c):
    return "m%d_n%d_k%d_br%d_%s" % (c[0], c[1], c[2], c[3], "_".join(k for k in sorted(c[4]) if c[4][k] is True))


@pytest.mark.parametrize("case", F32_FAST, ids=_id)
def test_poisoned_f32_fast(rt, case):
    m, n, k, br, kw = case
    gemm_case(rt, F32, m, n, k, br, seed=m + n + k + br, poison=True, **kw)


@pytest.mark.parametrize("case", BF16_CASES, ids=lambda c: "m%d_n%d_k%d_br%d" % c[:4])
def test_poisoned_bf16_vnni_fast(rt, case):
    m, n, k, br, kw = case
    blocks = [(0, 48), (m // 2 - 16, 40), (m - 40, 40)] if m * n * k * br > 2 ** 31 else None
    gemm_case(rt, BF16, m, n, k, br, vnni=True, seed=m + n, row_blocks=blocks, poison=True, **kw)


@pytest.mark.parametrize("case", BF16_FORCED, ids=lambda c: "v%d_m%d_n%d_k%d_br%d" % c[:5])
def test_poisoned_bf16_forced(rt, case):
    v, m, n, k, br, kw = case
    gemm_case(rt, BF16, m, n, k, br, vnni=True, seed=v * 1000 + m + n + br, force=v, poison=True, **kw)


@pytest.mark.parametrize("case", BF16_SMALL, ids=lambda c: "m%d_n%d_k%d_br%d" % c[:4])
def test_poisoned_bf16_small(rt, case):
    m, n, k, br, kw = case
    gemm_case(rt, BF16, m, n, k, br, vnni=True, seed=m + n + k + br, poison=True, **kw)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_poisoned_generic_ragged(rt, dt, shape):
    m, n, k, br = shape
    for mode in ("device", "host"):
        gemm_case(rt, dt, m, n, k, br, lda=k + 3, ldb=n + 1, ldc=n + 2, offs=(1, 2, 3, 1), seed=sum(shape), bias=(m % 2 == 1),
                  relu=(n % 2 == 1), beta0=(k % 2 == 0), mode=mode, vnni=(dt == BF16 and k % 2 == 0), poison=True)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("shape", [(64, 48, 64, 4), (32, 48, 32, 3), (40, 48, 32, 2), (72, 100, 96, 2), (8, 4, 32, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_poisoned_ragged_vector_loads(rt, dt, shape):
    m, n, k, br = shape
    for i, kw in enumerate((dict(beta0=True, bias=True), dict(ldc=n + 8, lda=k + 8, ldb=n + 4, offs=(8, 8, 4, 4)))):
        gemm_case(rt, dt, m, n, k, br, vnni=(dt == BF16), seed=sum(shape) + i, force=8, poison=True, expect="grouped", **kw)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6, 7, 9, 10])
def test_poisoned_f32_chunk_stream_lengths(rt, variant):
    m, n = (256, 128) if variant in (3, 10) else (128, 128)
    for k, br in ((64, 0), (64, 1), (64, 2), (64, 3), (64, 5), (64, 7), (128, 3), (192, 2), (64, 16)):
        for beta0 in (True, False):
            gemm_case(rt, F32, m, n, k, br, lda=k * max(br, 1) + 8, ldb=n + 4, ldc=n + 4, sa=k, sb=k * (n + 4), beta0=beta0,
                      bias=not beta0, relu=False, seed=variant * 100 + k + br, force=variant, offs=(4, 8, 4, 4), poison=True,
                      expect="fast")


@pytest.mark.parametrize("variant", [20, 21, 22, 23, 24, 25, 26, 27])
def test_poisoned_bf16_lw_chunk_stream_lengths(rt, variant):
    tiles = {0: (32, 64), 1: (64, 64), 2: (64, 128), 3: (128, 128)}
    bm, bn = tiles[(variant - 20) % 4]
    m, n = 2 * bm, 2 * bn
    for k, br in ((64, 1), (64, 3), (64, 8), (128, 5)):
        for beta0 in (True, False):
            gemm_case(rt, BF16, m, n, k, br, lda=k * br + 8, ldb=n + 8, ldc=n + 8, sa=k, sb=k * (n + 8), beta0=beta0, bias=not beta0,
                      vnni=variant < 24, seed=variant * 100 + k + br, force=variant, offs=(8, 16, 8, 8), poison=True, expect="lw")


@pytest.mark.parametrize("variant", [11, 28, 29, 30, 31])
def test_poisoned_lw16_and_vnni4(rt, variant):
    if variant == 11:
        for (m, n, k, br, kw) in ((64, 48, 64, 3, dict(bias=True)), (128, 96, 128, 2, dict(beta0=True, bias=True, lda=300, ldb=100,
                                                                                              ldc=104, offs=(4, 8, 4, 4)))):
            gemm_case(rt, F32, m, n, k, br, seed=m + br, force=11, poison=True, expect="lw16", **kw)
        return
    tiles = {28: (32, 64), 29: (64, 64), 30: (64, 128), 31: (128, 128)}
    bm, bn = tiles[variant]
    old = rt.set_vnni_factor(4), orc.set_vnni_factor(4)
    try:
        for k, br in ((64, 1), (64, 5), (128, 3)):
            for beta0 in (True, False):
                gemm_case(rt, BF16, 2 * bm, 2 * bn, k, br, lda=k * br + 8, ldb=2 * bn + 8, ldc=2 * bn + 8, sa=k, sb=k * (2 * bn + 8),
                          beta0=beta0, bias=True, vnni=True, seed=variant + k + br, force=variant, offs=(8, 16, 8, 8), poison=True,
                          expect="vnni4")
    finally:
        rt.set_vnni_factor(old[0])
        orc.set_vnni_factor(old[1])


@pytest.mark.parametrize("shape", [(6, 6, 6, 2), (32, 32, 32, 4), (64, 48, 64, 3), (10, 7, 4, 1), (128, 256, 64, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_poisoned_vnni_a_and_vnni_c(rt, shape):
    m, n, k, br = shape
    for xflags, kw in ((4096, dict()), (8192, dict(beta0=True, bias=True, relu=True)), (4096 | 8192, dict()), (8192, dict(bias=True))):
        if xflags & 8192 and m % 2:
            continue
        gemm_case(rt, BF16, m, n, k, br, lda=k + 2, ldb=n + 1, ldc=n + 3, offs=(2, 2, 3, 1), vnni=True, xflags=xflags, poison=True,
                  seed=sum(shape) + xflags, **kw)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("chunk", range(2))
def test_poisoned_random_dispatches(rt, dt, chunk):
    from test_parity_gpu import _random_gemm_case as draw
    rng = np.random.default_rng(5000 + 1000 * dt + chunk)
    for i in range(14):
        c = draw(rng, dt)
        gemm_case(rt, dt, seed=chunk * 100 + i, mode="device" if i % 4 else "host", poison=True, **c)


SPLIT_CASES = [(128, 1024, 64, 64, 9, True, False, False), (128, 768, 64, 36, 9, False, True, False), (64, 96, 64, 5, 7, True, False, False)]


@pytest.mark.parametrize("m,n,k,br,force,beta0,bias,relu", SPLIT_CASES)
def test_poisoned_split_launches(rt, m, n, k, br, force, beta0, bias, relu):
    try:
        for S in (1, 2, 3, 4, 5, 8, 16):
            rt.force_split(S)
            gemm_case(rt, F32, m, n, k, br, lda=k * br + 4, sa=k, sb=k * n, beta0=beta0, bias=bias, relu=relu, force=force, seed=S,
                      offs=(4, 8, 4, 4), poison=True)
    finally:
        rt.force_split(-1)


def test_poisoned_overlapping_batches(rt):
    gemm_case(rt, F32, 64, 64, 64, 6, lda=512, sa=64, sb=64, ldb=128, seed=9, poison=True)
    gemm_case(rt, BF16, 4, 4, 4, 64, sa=8, sb=8, vnni=True, seed=10, poison=True)
    gemm_case(rt, BF16, 160, 224, 80, 7, sa=16, sb=32, lda=320, ldb=224, beta0=True, vnni=True, seed=11, poison=True)


def test_poisoned_tile_queue_layer(rt):
    """32x32x32 f32 tile invokes over packed blocks with gaps between the blocks and poisoned tails: the grouped launch reads only the
    blocks"""
    MB, NB, KB, t, gap = 4, 8, 6, 32, 8
    blk = t * t + gap
    rng = np.random.default_rng(77)
    A = ed.poison_fill(MB * KB * blk + 64, F32)
    W = ed.poison_fill(NB * KB * blk + 64, F32)
    for arr, nb in ((A, MB * KB), (W, NB * KB)):
        for b in range(nb):
            arr[b * blk:b * blk + t * t] = rng.uniform(-1, 1, t * t).astype(np.float32)
    bias = ed.poison_fill(NB * t + 64, F32)
    bias[:NB * t] = rng.uniform(-1, 1, NB * t).astype(np.float32)
    C0 = ed.poison_fill(MB * NB * t * t + 64, F32)
    disp = (F32, t, t, t, t, t, t, blk, blk, 4, 0, 5, 4, 1)
    ref = C0.copy()
    old_async, old_q = rt.set_async(True), rt.set_tile_queue(1)
    try:
        h = rt.fused_brgemm_dispatch(*disp)
        dA, dW, dB, dC = dev(A), dev(W), dev(bias), dev(C0)
        for i in range(MB):
            for j in range(NB):
                orc.fused_brgemm(*disp, A, i * KB * blk, W, j * KB * blk, ref, (i * NB + j) * t * t, bias, j * t, KB)
                rt.fused_brgemm(F32, h, dA, i * KB * blk, dW, j * KB * blk, dC, (i * NB + j) * t * t, dB, j * t, KB)
        rt.synchronize()
        name = rt.last_grouped_kernel()
    finally:
        rt.synchronize()
        rt.set_tile_queue(old_q)
        rt.set_async(old_async)
    got = host(dC, C0)
    live = MB * NB * t * t
    assert np.isfinite(ref[:live]).all()
    from test_parity_gpu import check_close
    check_close(got[:live], ref[:live], F32, "poisoned queued layer [%s]" % name)
    assert np.array_equal(ed.bits(got[live:]), ed.bits(C0[live:]))
    assert "grouped" in name, name


@pytest.mark.parametrize("variant,m,dims", [(20, 128, [256, 256, 256]), (23, 256, [256, 256, 256])], ids=lambda v: str(v).replace(" ", ""))
def test_poisoned_bf16_chain_input_padding(rt, variant, m, dims):
    """the chain's input activation with NaN in its padding columns (Chain.new_input leaves them zero)"""
    from test_chain_gpu import Chain, run_chain_steps
    ch = Chain(rt, m, dims, seed=variant, force=variant, pad=8)
    plain = ch.new_input

    def new_input():
        x = plain()
        x.reshape(m, ch.ld[0])[:, dims[0]:] = ed.BF16_NAN
        return x
    ch.new_input = new_input
    run_chain_steps(rt, ch, 2, variant)


@pytest.mark.parametrize("variant,m,dims", [(7, 128, [256, 256, 256]), (6, 128, [128, 256, 256])], ids=lambda v: str(v).replace(" ", ""))
def test_poisoned_f32_chain_input_padding(rt, variant, m, dims):
    """Chain32's input activation with NaN / inf in its padding columns"""
    from test_chain_f32_gpu import Chain32, run_steps
    ch = Chain32(rt, m, dims, seed=variant, force=variant, pad=8)
    plain = ch.new_input

    def new_input():
        x = plain()
        pad = x.reshape(m, ch.ld[0])[:, dims[0]:]
        pad[:] = ed.poison_fill(pad.size, F32).reshape(pad.shape)
        return x
    ch.new_input = new_input
    run_steps(rt, ch, 2)
