"""The opt-in bf16x6 f32 GEMM arithmetic (xsmm_hip_set_f32_precision(6) / TPP_HIP_F32_PRECISION=bf16x6): every f32
operand split into three bf16 parts, six part products on the bf16 MFMA. Handles keep the mode they were dispatched with; shapes the
split kernel does not take run on the exact kernel of mode 0. Results are held to the project's f32 bar (check_close with the
element-wise floor and the fp64 truth), are bit-reproducible, and do not depend on the tile queue.
The split kernel does not beat the exact one yet, so the planner runs it only where a split tile is forced
(xsmm_hip_force_variant 12 .. 15, X6 below); these tests force the tile."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as orc
from test_parity_gpu import F32, check_close, dev, gemm_case, host, rand

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    old = r.set_f32_precision(6)
    assert old == 0
    try:
        yield r
    finally:
        r.set_f32_precision(0)  # process-wide: the tests after this module dispatch exact f32 again


X6 = {"64x64": 12, "64x32": 13, "32x32": 14, "128x64": 15}  # forced variants of the split tiles


def x6_tile(m, n):
    return X6["64x64"] if m % 64 == 0 and n % 64 == 0 else X6["64x32"] if m % 64 == 0 else X6["32x32"]


def forced(rt, v, fn):
    rt.force_variant(v)
    try:
        return fn()
    finally:
        rt.force_variant(-1)


def c2_dispatch(rt, flags=0, force=X6["64x64"]):
    return forced(rt, force, lambda: rt.brgemm_dispatch(F32, 1024, 1024, 64, 1024, 1024, 1024, 64, 65536, flags))


def test_default_mode_and_handles(rt):
    code = "import importlib, sys; sys.path.insert(0, %r); r = importlib.import_module('tpp-mlir_amd').get_runtime(); print(r.get_f32_precision())" % ROOT
    env = dict(os.environ)
    env.pop("TPP_HIP_F32_PRECISION", None)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "0"
    assert rt.get_f32_precision() == 6
    h6 = c2_dispatch(rt)
    assert "bf16x6" in rt.kernel_name(h6)
    assert rt.kernel_name(c2_dispatch(rt, force=-1)) == "brgemm_f32_fast_lw<64x64,k2>"  # unforced: the exact plan
    assert rt.set_f32_precision(3) == -1 and rt.get_f32_precision() == 6
    rng = np.random.default_rng(5)
    A, B, C = (rand(rng, 1024 * 1024, F32) for _ in range(3))
    dA, dB = dev(A), dev(B)
    d1 = dev(C)
    rt.brgemm(F32, h6, dA, 0, dB, 0, d1, 0, 16)
    assert rt.set_f32_precision(0) == 6
    try:
        h0 = c2_dispatch(rt)
        assert h0 != h6
        assert rt.kernel_name(h0) == "brgemm_f32_fast_lw<64x64,k2>"  # today's exact plan of C2 (a forced split tile needs mode 6)
        assert "bf16x6" in rt.kernel_name(h6)  # the handle keeps its mode
        d2 = dev(C)
        rt.brgemm(F32, h6, dA, 0, dB, 0, d2, 0, 16)
        d3 = dev(C)
        rt.brgemm(F32, h0, dA, 0, dB, 0, d3, 0, 16)
        import torch
        assert torch.equal(d1, d2)      # still the split kernel after the setting went back to 0
        assert not torch.equal(d1, d3)  # ... which is not the exact kernel's arithmetic
    finally:
        assert rt.set_f32_precision(6) == 0
    assert c2_dispatch(rt) == h6


@pytest.mark.parametrize("value,mode", [("bf16x6", 6), ("6", 6), ("bf16x3", 0), ("", 0)])
def test_environment_variable(value, mode):
    code = ("import importlib, sys; sys.path.insert(0, %r); r = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(r.get_f32_precision())" % ROOT)
    env = dict(os.environ)
    env["TPP_HIP_F32_PRECISION"] = value
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == str(mode)


def test_c2_full_size_bf16x6(rt):
    import torch
    m = n = 1024
    k, br = 64, 16
    gen = orc.TensorInit("normal", 123)
    for trial, (A, B, C) in enumerate([
            (gen.fill(m * 1024), gen.fill(1024 * n), gen.fill(m * n)),
            tuple(rand(np.random.default_rng(s), 1024 * 1024, F32) for s in (1, 2, 3))]):
        ref = C.copy()
        orc.fused_brgemm_omp(F32, m, n, k, 1024, 1024, 1024, 64, 65536, 0, 0, 0, A, B, ref, None, br)
        h = c2_dispatch(rt)
        assert "bf16x6" in rt.kernel_name(h)
        dA, dB, dC = dev(A), dev(B), dev(C)
        rt.brgemm(F32, h, dA, 0, dB, 0, dC, 0, br)
        got = host(dC, C)
        truth = C.astype(np.float64).reshape(m, n) + A.astype(np.float64).reshape(m, 1024) @ B.astype(np.float64).reshape(1024, n)
        mag = np.abs(C).astype(np.float64).reshape(m, n) + np.abs(A).astype(np.float64).reshape(m, 1024) @ np.abs(B).astype(np.float64).reshape(1024, n)
        check_close(got, ref, F32, "C2 bf16x6 trial %d" % trial, mag=mag.reshape(-1), K=1024, truth=truth.reshape(-1))
        dC2 = dev(C)
        rt.brgemm(F32, h, dA, 0, dB, 0, dC2, 0, br)
        assert torch.equal(dC, dC2)  # bit-reproducible
        h0 = c2_dispatch(rt, 4)
        assert "bf16x6" in rt.kernel_name(h0)
        dZ = dev(np.zeros_like(C))
        rt.brgemm(F32, h0, dA, 0, dB, 0, dZ, 0, br)
        alt = host(dZ, C).astype(np.float64) + C
        assert np.abs(alt - got).max() <= 1e-5 * max(1.0, np.abs(got).max())


def test_c3_fused_layer_bf16x6(rt):
    m, n, k, br = 512, 1024, 64, 16
    gen = orc.TensorInit("normal", 123)
    A, W, bias = gen.fill(m * 1024), gen.fill(1024 * n), gen.fill(n)
    A -= np.float32(0.08)
    C = np.full(m * n, np.float32(7.0))
    ref = C.copy()
    orc.fused_brgemm_omp(F32, m, n, k, 1024, 1024, 1024, 64, 65536, 4, 5, 1, A, W, ref, bias, br)
    h = forced(rt, X6["64x32"], lambda: rt.fused_brgemm_dispatch(F32, m, n, k, 1024, 1024, 1024, 64, 65536, 4, 0, 5, 4, 1))
    assert "bf16x6" in rt.kernel_name(h)
    dC = dev(C)
    rt.fused_brgemm(F32, h, dev(A), 0, dev(W), 0, dC, 0, dev(bias), 0, br)
    got = host(dC, C)
    truth = np.maximum(A.astype(np.float64).reshape(m, 1024) @ W.astype(np.float64).reshape(1024, n) + bias.astype(np.float64), 0.0)
    mag = np.abs(A).astype(np.float64).reshape(m, 1024) @ np.abs(W).astype(np.float64).reshape(1024, n) + np.abs(bias).astype(np.float64)
    check_close(got, ref, F32, "C3 bf16x6", mag=mag.reshape(-1), K=1024, truth=truth.reshape(-1))
    assert (got >= 0).all() and (got == 0).any()


SWEEP = [
    # (m, n, k, br, kwargs, split kernel expected); the split tile forced is x6_tile's (128x64 where the kwargs say so)
    (512, 512, 64, 1, dict(), True),
    (512, 1024, 128, 3, dict(beta0=True), True),
    (96, 64, 64, 2, dict(relu=True), True),                                            # 32x32 + K4
    (512, 512, 1024, 1, dict(), True),
    (2048, 1024, 64, 2, dict(beta0=True, force=X6["128x64"]), True),
    (512, 512, 64, 16, dict(lda=1028, ldb=516, ldc=520, sa=64, sb=64 * 516, bias=True, relu=True), True),
    (384, 512, 128, 3, dict(ldc=516, offs=(4, 8, 3, 1)), True),
    (512, 384, 64, 3, dict(lda=72, offs=(3, 1, 2, 0), beta0=True, bias=True), True),   # unaligned A / B: the element loads
    (48, 4096, 64, 3, dict(), False),                                                  # m not a multiple of 32
    (512, 512, 32, 4, dict(), False),                                                  # k not a multiple of 64
    (512, 512, 64, 2, dict(lda=66, sa=64 * 66), False),                                # lda not a multiple of 4
    (128, 1024, 64, 16, dict(lda=1024, ldb=1024, sa=64, sb=65536), True),              # skinny (the exact plan: 32x16 tiles)
    (128, 1024, 64, 16, dict(lda=1024, ldb=1024, sa=64, sb=65536, force=-1), False),   # ... not forced: the exact plan
]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "%dx%dx%d_br%d" % c[:4])
def test_bf16x6_shape_sweep(rt, case):
    m, n, k, br, kw, split = case
    kw = dict(kw)
    force = kw.pop("force", x6_tile(m, n))
    kw["force"] = None if force < 0 else force
    name = gemm_case(rt, F32, m, n, k, br, **kw)
    assert ("bf16x6" in name) == split, name
    if not split:
        rt.set_f32_precision(0)
        try:
            name0 = gemm_case(rt, F32, m, n, k, br, **kw)
        finally:
            rt.set_f32_precision(6)
        assert name == name0


def test_bf16x6_plain_gemm(rt):
    rng = np.random.default_rng(11)
    m, n, k = 384, 512, 256
    A, B, C = rand(rng, m * k, F32), rand(rng, k * n, F32), rand(rng, m * n, F32)
    ref = C.copy()
    orc.gemm(F32, m, n, k, k, n, n, 0, A, 0, B, 0, ref, 0)
    h = forced(rt, x6_tile(m, n), lambda: rt.gemm_dispatch(F32, m, n, k, k, n, n, 0))
    assert "bf16x6" in rt.kernel_name(h)
    dC = dev(C)
    rt.gemm(F32, h, dev(A), 0, dev(B), 0, dC, 0)
    mag = np.abs(C).astype(np.float64) + (np.abs(A).astype(np.float64).reshape(m, k) @ np.abs(B).astype(np.float64).reshape(k, n)).reshape(-1)
    check_close(host(dC, C), ref, F32, "gemm bf16x6", mag=mag, K=k)


def test_bf16x6_split_exactness(rt):
    """A a permutation matrix, B over many binades: C = P B up to the split's representation error (about 2^-27): within 1 ulp"""
    m = n = k = 512
    rng = np.random.default_rng(3)
    perm = rng.permutation(k)
    A = np.zeros((m, k), np.float32)
    A[np.arange(m), perm] = 1.0
    B = (10.0 ** rng.uniform(-30, 30, (k, n)) * rng.choice([-1.0, 1.0], (k, n))).astype(np.float32)
    h = forced(rt, X6["64x64"], lambda: rt.brgemm_dispatch(F32, m, n, k, k, n, n, 0, 0, 4))
    assert "bf16x6" in rt.kernel_name(h)
    dC = dev(np.zeros(m * n, np.float32))
    rt.brgemm(F32, h, dev(A.reshape(-1)), 0, dev(B.reshape(-1)), 0, dC, 0, 1)
    got = host(dC, np.zeros(1, np.float32)).reshape(m, n)
    want = B[perm]
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert (np.sign(got) == np.sign(want)).all()
    assert ulps.max() <= 1, "worst %d ulp" % ulps.max()
    print("bf16x6 split exactness: %.4f of the elements bit-exact, worst %d ulp" % ((ulps == 0).mean(), ulps.max()))


def test_bf16x6_special_values(rt):
    m = n = 512
    k = 128
    rng = np.random.default_rng(9)
    A = rand(rng, m * k, F32).reshape(m, k)
    B = rand(rng, k * n, F32).reshape(k, n)
    B[::7, ::5] = 0.5  # values exactly representable in bf16 (mid = lo = 0)
    A[3, 10] = np.inf
    A[17, 20] = -np.inf
    A[30, 40] = np.nan
    B[50, 7] = np.inf
    B[60, 9] = np.nan
    A[40, 5] = np.float32(3.4e38)  # finite, above the bf16 range
    A[41, 6] = np.finfo(np.float32).max
    B[70, 33] = np.float32(-3.39e38)
    outs = []
    for mode in (0, 6):
        rt.set_f32_precision(mode)
        try:
            h = forced(rt, X6["64x64"], lambda: rt.brgemm_dispatch(F32, m, n, k, k, n, n, 0, 0, 4))
        finally:
            rt.set_f32_precision(6)
        assert ("bf16x6" in rt.kernel_name(h)) == (mode == 6)
        dC = dev(np.zeros(m * n, np.float32))
        rt.brgemm(F32, h, dev(A.reshape(-1)), 0, dev(B.reshape(-1)), 0, dC, 0, 1)
        outs.append(host(dC, np.zeros(1, np.float32)).reshape(m, n))
    ex, x6 = outs
    assert (~np.isfinite(ex)).any() and np.isfinite(ex).any()
    assert np.array_equal(np.isnan(ex), np.isnan(x6))
    assert np.array_equal(np.isposinf(ex), np.isposinf(x6))
    assert np.array_equal(np.isneginf(ex), np.isneginf(x6))
    fin = np.isfinite(ex)
    assert np.abs(ex[fin] - x6[fin]).max() <= 1e-5 * np.abs(ex[fin]).max()
    # a tile without non-finite operands but with values near FLT_MAX runs the split path proper
    A2 = rand(rng, m * k, F32).reshape(m, k)
    A2[5, 3] = np.finfo(np.float32).max
    A2[6, 4] = np.float32(-3.4e38)
    B2 = rand(rng, k * n, F32).reshape(k, n) * np.float32(0.5)
    res = []
    for mode in (0, 6):
        rt.set_f32_precision(mode)
        try:
            h = forced(rt, X6["64x64"], lambda: rt.brgemm_dispatch(F32, m, n, k, k, n, n, 0, 0, 4))
        finally:
            rt.set_f32_precision(6)
        dC = dev(np.zeros(m * n, np.float32))
        rt.brgemm(F32, h, dev(A2.reshape(-1)), 0, dev(B2.reshape(-1)), 0, dC, 0, 1)
        res.append(host(dC, np.zeros(1, np.float32)).reshape(m, n))
    assert np.isfinite(res[0]).all() and np.isfinite(res[1]).all()
    assert np.abs(res[0] - res[1]).max() <= 1e-5 * np.abs(res[0]).max()
    # finite operands whose products overflow (hi.hi and hi.mid could reach infinities of both signs): the same infinities as exact
    A3 = rand(rng, m * k, F32).reshape(m, k)
    B3 = rand(rng, k * n, F32).reshape(k, n)
    A3[100, 7] = np.float32(3.0e38)
    A3[101, 7] = np.float32(-2.9e38)
    B3[7, 200] = np.float32(4.0e9)
    B3[7, 201] = np.float32(-3.7e9)
    res = []
    for mode in (0, 6):
        rt.set_f32_precision(mode)
        try:
            h = forced(rt, X6["64x64"], lambda: rt.brgemm_dispatch(F32, m, n, k, k, n, n, 0, 0, 4))
        finally:
            rt.set_f32_precision(6)
        dC = dev(np.zeros(m * n, np.float32))
        rt.brgemm(F32, h, dev(A3.reshape(-1)), 0, dev(B3.reshape(-1)), 0, dC, 0, 1)
        res.append(host(dC, np.zeros(1, np.float32)).reshape(m, n))
    ex, x6 = res
    assert (~np.isfinite(ex)).any()
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(ex), f(x6))


def test_bf16x6_tile_queue(rt):
    """Tile-queue-sized invokes under mode 6: planned on the exact skinny tiles (a fallback), they are queued and grouped exactly as under
    mode 0 - same kernels, same bits. A split-kernel handle interleaved with them is handed over ungrouped: its result is the same with the
    queue on and off."""
    import torch
    rng = np.random.default_rng(21)
    m = n = 64
    k, br, tiles = 128, 2, 24
    A = rand(rng, tiles * m * k * br, F32)
    B = rand(rng, k * br * n, F32)
    C = rand(rng, tiles * m * n, F32)
    AL, BL, CL = rand(rng, 512 * 256, F32), rand(rng, 256 * 512, F32), rand(rng, 512 * 512, F32)
    dA, dB, dAL, dBL = dev(A), dev(B), dev(AL), dev(BL)
    hl = forced(rt, X6["64x64"], lambda: rt.brgemm_dispatch(F32, 512, 512, 64, 64 * 4, 512, 512, 64, 64 * 512, 0))
    assert "bf16x6" in rt.kernel_name(hl)
    names, res = [], {}
    for mode, queue in ((0, 1), (6, 1), (6, 0)):
        rt.set_f32_precision(mode)
        try:
            h = rt.brgemm_dispatch(F32, m, n, k, k, n, n, m * k, k * n, 0)
        finally:
            rt.set_f32_precision(6)
        names.append(rt.kernel_name(h))
        prev_async = rt.set_async(bool(queue))
        prev_q = rt.set_tile_queue(queue)
        try:
            launches0 = rt.tile_queue_stats()[0]
            dC, dCL = dev(C), dev(CL)
            for rep in range(2):
                for t in range(tiles):
                    rt.brgemm(F32, h, dA, t * m * k * br, dB, 0, dC, t * m * n, br)
                    if t % 8 == 3:
                        rt.brgemm(F32, hl, dAL, 0, dBL, 0, dCL, 0, 4)
            rt.synchronize()
            grouped = rt.tile_queue_stats()[0] - launches0
        finally:
            rt.set_tile_queue(prev_q)
            rt.set_async(prev_async)
        if queue:
            assert grouped > 0, "mode %d: the tiles were not grouped" % mode
        res[(mode, queue)] = (dC, dCL)
    assert names[0] == names[1] and "bf16x6" not in names[1]
    assert torch.equal(res[(0, 1)][0], res[(6, 1)][0])   # the fallback handle goes the way of mode 0
    assert torch.equal(res[(6, 1)][1], res[(6, 0)][1])   # the split handle: queue on == queue off
    assert torch.equal(res[(0, 1)][1], res[(6, 0)][1])
