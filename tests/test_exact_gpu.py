"""Every GEMM kernel BIT-EXACT against the oracle on exact inputs (tests/exact_data.py): small integers times
powers of two, so that every correct kernel - whatever its tiling, K split, split-launch count, queue grouping or chain seam - holds
the oracle's f32 accumulator, and the stored result must be the oracle's bits (bf16: after the one round-to-nearest-even store).
Also: targeted bf16 rounding cases (ties, near-ties, double-rounding traps, store overflow), inf / NaN propagation, subnormal
operands, power-of-two scales, bf16x6 at small scales, and eltwise ops on special values. Each case asserts the kernel it reached;
test_zz_coverage checks that every variant 0 .. 31, the generic kernel, grouped / quad / merged-grid replays, split launches and both
chains were reached."""
import importlib

import numpy as np
import pytest

import exact_data as ed
from oracle import pyoracle as orc
from test_parity_gpu import BF16, F32, VB, check_close, dev, gemm_case, host

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")

# forced variant -> (dtype, m, n, kernel-name substring); bf16 VNNI-2 unless flat (24 .. 27); 28 .. 31 under VNNI factor 4
VARIANTS = {
    0: (F32, 128, 128, "brgemm_f32_fast<64x64,k1>"), 1: (F32, 128, 96, "brgemm_f32_fast<64x32,k2>"),
    2: (F32, 96, 96, "brgemm_f32_fast<32x32,k4>"), 3: (F32, 256, 128, "brgemm_f32_fast<128x64,k1>"),
    4: (F32, 128, 128, "brgemm_f32_fast<64x64,k2>"), 5: (F32, 128, 128, "brgemm_f32_fast_lw<64x64,k1>"),
    6: (F32, 128, 192, "brgemm_f32_fast_lw<64x64,k2>"), 7: (F32, 128, 96, "brgemm_f32_fast_lw<64x32,k4>"),
    8: (F32, 96, 72, "brgemm_grouped"), 9: (F32, 96, 96, "brgemm_f32_fast_lw<32x32,k4>"),
    10: (F32, 256, 128, "brgemm_f32_fast_lw<128x64,k1>"), 11: (F32, 64, 48, "brgemm_f32_lw16<32x16,k4>"),
    12: (F32, 128, 128, "brgemm_f32_bf16x6<64x64,k1>"), 13: (F32, 128, 96, "brgemm_f32_bf16x6<64x32,k2>"),
    14: (F32, 96, 96, "brgemm_f32_bf16x6<32x32,k4>"), 15: (F32, 256, 128, "brgemm_f32_bf16x6<128x64,k1>"),
    16: (BF16, 128, 192, "brgemm_bf16_fast<64x64>"), 17: (BF16, 128, 256, "brgemm_bf16_dma<128x128>"),
    18: (BF16, 256, 256, "brgemm_bf16_dma<256x256>"), 19: (BF16, 64, 96, "brgemm_bf16_small<32x32,k4>"),
    20: (BF16, 64, 128, "brgemm_bf16_lw<32x64,k2>"), 21: (BF16, 128, 128, "brgemm_bf16_lw<64x64>"),
    22: (BF16, 128, 256, "brgemm_bf16_lw<64x128>"), 23: (BF16, 256, 256, "brgemm_bf16_lw<128x128>"),
    24: (BF16, 64, 128, "brgemm_bf16_lw_flatb<32x64,k2>"), 25: (BF16, 128, 128, "brgemm_bf16_lw_flatb<64x64>"),
    26: (BF16, 128, 256, "brgemm_bf16_lw_flatb<64x128>"), 27: (BF16, 256, 256, "brgemm_bf16_lw_flatb<128x128>"),
    28: (BF16, 64, 128, "brgemm_bf16_lw_vnni4<32x64,k2>"), 29: (BF16, 128, 128, "brgemm_bf16_lw_vnni4<64x64>"),
    30: (BF16, 128, 256, "brgemm_bf16_lw_vnni4<64x128>"), 31: (BF16, 256, 256, "brgemm_bf16_lw_vnni4<128x128>"),
}
SEEN = {}  # coverage label -> kernel names reached


def seen(label, name):
    SEEN.setdefault(label, set()).add(name)
    return name


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


class variant_mode:
    """the process-wide settings a forced variant needs: bf16x6 for 12 .. 15, VNNI factor 4 (runtime and oracle) for 28 .. 31"""

    def __init__(self, rt, v):
        self.rt, self.v = rt, v

    def __enter__(self):
        self.old = None
        if 12 <= self.v <= 15:
            self.old = self.rt.set_f32_precision(6)
        if self.v >= 28:
            self.old = (self.rt.set_vnni_factor(4), orc.set_vnni_factor(4))
        return self

    def __exit__(self, *exc):
        if 12 <= self.v <= 15:
            self.rt.set_f32_precision(self.old)
        if self.v >= 28:
            self.rt.set_vnni_factor(self.old[0])
            orc.set_vnni_factor(self.old[1])


def variant_case(rt, v, dt=None, k=64, br=4, **kw):
    vdt, m, n, want = VARIANTS[v]
    dt = dt or vdt
    if v == 8 and dt == BF16:
        want = "brgemm_grouped"
    vnni = dt == BF16 and not (24 <= v <= 27)
    with variant_mode(rt, v):
        name = gemm_case(rt, dt, m, n, k, br, vnni=vnni, force=v, expect=want, **kw)
    return seen(v if v != 8 else "generic", name)


EPILOGUES = [
    dict(beta0=True),
    dict(bias=True, relu=True, mode="host"),
    dict(bias=True, lda=64 * 4 + 16, ldb=None, ldc=None, offs=(16, 16, 16, 16), sa=64),   # strided, batch along k of one A row
    dict(beta0=True, bias=True, relu=True, poison=True, offs=(16, 32, 16, 16)),
]


def _strided(kw, n):
    kw = dict(kw)
    if "ldb" in kw:
        kw["ldb"], kw["ldc"] = n + 16, n + 16
        kw["sb"] = 64 * (n + 16)
    return kw


@pytest.mark.parametrize("v", sorted(VARIANTS))
def test_exact_every_variant(rt, v):
    """every forced variant, beta 0 / 1, bias, relu, host and device pointers, strides and offsets, poisoned surroundings"""
    n = VARIANTS[v][2]
    for i, kw in enumerate(EPILOGUES):
        kw = _strided(kw, n)
        if 12 <= v <= 15:  # operands of up to 16 significant bits: the split's mid parts are live, and still exact
            kw["ranges"] = (2 ** 15 - 1, 1, 2 ** 20) if i % 2 == 0 else (1, 2 ** 15 - 1, 2 ** 20)
        variant_case(rt, v, seed=v * 10 + i, values="exact", **kw)
    if v == 8:
        for i, kw in enumerate(EPILOGUES):
            variant_case(rt, v, dt=BF16, seed=v * 10 + i + 5, values="exact", **_strided(kw, VARIANTS[v][2]))


@pytest.mark.parametrize("shape", [(6, 6, 6, 2), (32, 32, 32, 4), (64, 48, 64, 3), (10, 8, 4, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("xflags", [4096, 8192, 4096 | 8192])
def test_exact_vnni_a_and_vnni_c(rt, shape, xflags):
    m, n, k, br = shape
    for i, kw in enumerate((dict(beta0=False), dict(beta0=True, bias=True, relu=True, mode="host"), dict(bias=True, poison=True))):
        name = gemm_case(rt, BF16, m, n, k, br, lda=k + 2, ldb=n + 1, ldc=n + 3, offs=(2, 2, 3, 1), vnni=True, xflags=xflags,
                         values="exact", seed=sum(shape) + i, **kw)
        seen("vnni_a_c", name)


# ---------------------------------------------------------------- targeted bf16 rounding cases
BF16_VARIANTS = [8] + list(range(16, 32))


def _run_given(rt, v, A, B, C, D, m, n, k, beta0, bias, relu, mode="device"):
    """one forced-variant dispatch on given flat bf16 operands (A [m][k], B [k][n] - packed to the variant's layout here)"""
    vnni = not (24 <= v <= 27)
    with variant_mode(rt, v):
        vf = orc.lib().oracle_get_vnni_factor()
        Bp = orc.pack_vnni(B, k, n, vf) if vnni else B
        flags = (4 if beta0 else 0) | (VB if vnni else 0)
        ep = (0, 5 if relu else 0, 4 if bias else 0, 1 if bias else 0)
        ref = C.copy()
        orc.fused_brgemm(BF16, m, n, k, k, n, n, 0, 0, flags, *ep, A, 0, Bp, 0, ref, 0, D, 0, 1)
        rt.force_variant(v)
        try:
            h = rt.fused_brgemm_dispatch(BF16, m, n, k, k, n, n, 0, 0, flags, *ep)
        finally:
            rt.force_variant(-1)
        name = rt.kernel_name(h)
        if mode == "device":
            dC = dev(C)
            rt.fused_brgemm(BF16, h, dev(A), 0, dev(Bp), 0, dC, 0, dev(D), 0, 1)
            got = host(dC, C)
        else:
            got = C.copy()
            rt.fused_brgemm(BF16, h, A, 0, Bp, 0, got, 0, D, 0, 1)
    return name, got, ref


@pytest.mark.parametrize("v", BF16_VARIANTS)
def test_exact_bf16_rounding_cases(rt, v):
    """ties and near-ties at both signs, C + acc and bias + acc that are ties only if acc were rounded first, and the store's overflow
    edge (0x7f7f stays finite, the halfway point to 2^128 and above give inf, one f32 ulp below stays finite) - bit for bit"""
    _, m, n, want = VARIANTS[v] if v != 8 else (BF16, 96, 72, "grouped")
    k = 64
    A, B, C, D = ed.rounding_case(m, n, k)
    for beta0, bias, relu, mode in ((False, True, False, "device"), (True, True, False, "host"), (False, False, True, "device")):
        name, got, ref = _run_given(rt, v, A, B, C, D, m, n, k, beta0, bias, relu, mode)
        assert want in name, (want, name)
        seen(v if v != 8 else "generic", name)
        ed.check_bits(got, ref, BF16, "rounding cases [%s] beta0=%d bias=%d relu=%d" % (name, beta0, bias, relu), special=True)
        assert np.isposinf(ed.as_f32(ref)).any() and (ed.bits(ref) == 0x7f7f).any()


# ---------------------------------------------------------------- inf / NaN, scales, subnormals
SPECIAL_VARIANTS = [0, 2, 3, 5, 7, 8, 9, 10, 11, 12, 16, 17, 18, 19, 20, 23, 24, 28]


@pytest.mark.parametrize("v", SPECIAL_VARIANTS)
def test_exact_special_values(rt, v):
    """inf, -inf and NaN in A, B, C (beta = 1) and the bias, exact data elsewhere: the same NaN / +inf / -inf pattern as the oracle,
    finite elements bit for bit; relu of NaN is 0 as in the oracle's x > 0 ? x : 0"""
    for i, kw in enumerate((dict(bias=True), dict(bias=True, relu=True), dict(beta0=True, bias=True, mode="host"))):
        variant_case(rt, v, seed=300 + v * 10 + i, values="special", **kw)


SCALES = [(-60, -60), (-30, -30), (40, 20), (50, 50)]


@pytest.mark.parametrize("v", [0, 5, 8, 11, 12, 16, 18, 19, 21, 25, 30])
@pytest.mark.parametrize("scale", SCALES, ids=lambda s: "2^%d" % (s[0] + s[1]))
def test_exact_power_of_two_scales(rt, v, scale):
    """the exact data scaled by 2^s (A) and 2^t (B), C and bias by 2^(s+t), every value in the normal range: still bit-exact"""
    kw = dict(ranges=(2 ** 15 - 1, 1, 2 ** 20)) if 12 <= v <= 15 else {}
    variant_case(rt, v, seed=500 + v, values="exact", scale=scale, bias=True, **kw)
    variant_case(rt, v, seed=600 + v, values="exact", scale=scale, beta0=True, bias=True, relu=True, **kw)


@pytest.mark.parametrize("v", [0, 3, 5, 8, 9, 11])
def test_f32_subnormal_operands(rt, v):
    """A holds multiples of 2^-149 (subnormals), B small integers, every |sum| < 2^-125: every product and partial sum is exact on the
    subnormal grid, so no kernel may flush them (the code objects are built with denorm mode 3)"""
    _, m, n, want = VARIANTS[v]
    k, br = 64, 2
    rng = np.random.default_rng(v)
    A = np.ldexp(rng.integers(-255, 256, m * k * br).astype(np.float64), -149).astype(np.float32)
    B = rng.integers(-7, 8, k * br * n).astype(np.float32)
    C = np.ldexp(rng.integers(-2 ** 20, 2 ** 20, m * n).astype(np.float64), -149).astype(np.float32)
    assert (np.abs(A[A != 0]) < np.finfo(np.float32).tiny).all()
    with variant_mode(rt, v):
        for beta0 in (False, True):
            ref = C.copy()
            flags = 4 if beta0 else 0
            orc.brgemm(F32, m, n, k, k * br, n, n, k, k * n, flags, A, 0, B, 0, ref, 0, br)
            assert (np.abs(ref) < 2.0 ** -125).all() and (np.abs(ref[ref != 0]) < np.finfo(np.float32).tiny).any()
            rt.force_variant(v)
            try:
                h = rt.brgemm_dispatch(F32, m, n, k, k * br, n, n, k, k * n, flags)
            finally:
                rt.force_variant(-1)
            assert want in rt.kernel_name(h), rt.kernel_name(h)
            dC = dev(C)
            rt.brgemm(F32, h, dev(A), 0, dev(B), 0, dC, 0, br)
            ed.check_bits(host(dC, C), ref, F32, "subnormal A [%s] beta0=%d" % (rt.kernel_name(h), beta0))


@pytest.mark.parametrize("v", [8, 16, 17, 19, 20, 24, 28])
def test_bf16_subnormal_operands(rt, v):
    """bf16 A holds multiples of 2^-133 (bf16 subnormals), B small integers: results land on the bf16 subnormal grid (or between its
    points, rounded to nearest even) - the MFMA must not flush the inputs, the store must not flush the outputs"""
    _, m, n, want = VARIANTS[v] if v != 8 else (BF16, 96, 72, "grouped")
    k = 64
    rng = np.random.default_rng(v)
    A = orc.f32_to_bf16(np.ldexp(rng.integers(-7, 8, m * k).astype(np.float64), -133).astype(np.float32))
    B = orc.f32_to_bf16(rng.integers(-1, 2, k * n).astype(np.float32))
    C = orc.f32_to_bf16(np.ldexp(rng.integers(-127, 128, m * n).astype(np.float64), -133).astype(np.float32))
    D = np.zeros(n, np.uint16)
    assert (np.abs(ed.as_f32(A)[ed.as_f32(A) != 0]) < np.finfo(np.float32).tiny).all()
    for beta0 in (False, True):
        name, got, ref = _run_given(rt, v, A, B, C, D, m, n, k, beta0, False, False)
        assert want in name, name
        r = ed.as_f32(ref)
        assert (np.abs(r[r != 0]) < np.finfo(np.float32).tiny).mean() > 0.5
        ed.check_bits(got, ref, BF16, "bf16 subnormal A [%s] beta0=%d" % (name, beta0))


@pytest.mark.parametrize("e", [-60, -63, -66])
def test_bf16x6_small_scales_against_fp64(rt, e):
    """random (non-exact) f32 operands around 2^e each: the split's mid and lo part products fall below 2^-126. The result must be as
    close to the fp64 truth as the oracle is (the project's f32 bar, check_close(..., truth=)). (Below about 2^-66 the products
    themselves are subnormal: the exact path and the oracle lose bits too, and the f32 bar no longer applies to either.)"""
    m, n, k = 128, 128, 256
    rng = np.random.default_rng(-e)
    A = np.ldexp(rng.uniform(-1, 1, m * k), e).astype(np.float32)
    B = np.ldexp(rng.uniform(-1, 1, k * n), e).astype(np.float32)
    C = np.ldexp(rng.uniform(-1, 1, m * n), 2 * e).astype(np.float32)
    ref = C.copy()
    orc.brgemm(F32, m, n, k, k, n, n, 0, 0, 0, A, 0, B, 0, ref, 0, 1)
    truth = C.astype(np.float64) + (A.astype(np.float64).reshape(m, k) @ B.astype(np.float64).reshape(k, n)).reshape(-1)
    with variant_mode(rt, 12):
        rt.force_variant(12)
        try:
            h = rt.brgemm_dispatch(F32, m, n, k, k, n, n, 0, 0, 0)
        finally:
            rt.force_variant(-1)
        assert "bf16x6" in rt.kernel_name(h), rt.kernel_name(h)
        dC = dev(C)
        rt.brgemm(F32, h, dev(A), 0, dev(B), 0, dC, 0, 1)
    got = host(dC, C)
    s = 2.0 ** (-2 * e)  # compare at unit scale (the bar's absolute terms assume results of order 1); exact in fp64
    check_close((got.astype(np.float64) * s).astype(np.float32), (ref.astype(np.float64) * s).astype(np.float32), F32, "bf16x6 at 2^%d [%s]" % (e, rt.kernel_name(h)),
                truth=truth * s)


# ---------------------------------------------------------------- split launches
SPLIT_CASES = [
    (128, 1024, 64, 64, 9, True, False, False),
    (128, 768, 64, 36, 9, False, True, True),
    (128, 256, 64, 7, 6, False, True, False),
    (64, 96, 64, 5, 7, True, False, True),
    (96, 160, 128, 3, 9, False, False, False),
]


@pytest.mark.parametrize("m,n,k,br,force,beta0,bias,relu", SPLIT_CASES)
def test_exact_split_counts(rt, m, n, k, br, force, beta0, bias, relu):
    """every forced split count gives the oracle's bits: the partial sums in split scratch are exact, and must not be rounded"""
    refined = set()
    try:
        for S in (1, 2, 3, 4, 5, 8, 16):
            rt.force_split(S)
            gemm_case(rt, F32, m, n, k, br, lda=k * br, sa=k, sb=k * n, beta0=beta0, bias=bias, relu=relu, force=force,
                      values="exact", seed=S, offs=(4, 8, 4, 4), poison=S % 2 == 0)
            refined.add(rt.last_refined_kernel())
    finally:
        rt.force_split(-1)
    splits = {r for r in refined if "split" in r}
    assert splits, refined
    for r in splits:
        seen("split", r)


# ---------------------------------------------------------------- tile queue: grouped, quads, merged grid
def _queue_layer(rt, dt, M, N, K, t, vn, fc, passes, expect):
    """a layer as tile invokes over packed blocks (A [MB][KB][t][t], W [NB][KB][t][t] (bf16: VNNI-vn inside a block), C [MB][NB][t][t]),
    with poisoned tails behind every packed buffer; the oracle replays the same calls. Every pass bit-exact."""
    rng = np.random.default_rng(M + N + K + vn + fc)
    MB, NB, KB = M // t, N // t, K // t
    ra, rb, rc = ed.exact_ranges(dt, K * (1 if fc else passes))
    A = ed.exact_fill(rng, MB * KB * t * t + 64, dt, ra)
    W = ed.exact_fill(rng, NB * KB * t * t + 64, dt, rb)
    bias = ed.exact_fill(rng, N + 64, dt, rc)
    C0 = ed.exact_fill(rng, MB * NB * t * t + 64, dt, rc)
    for arr, live in ((A, MB * KB * t * t), (W, NB * KB * t * t), (bias, N), (C0, MB * NB * t * t)):
        arr[live:] = ed.poison_fill(arr.size - live, dt)
    if fc:
        C0[:MB * NB * t * t] = ed.poison_fill(MB * NB * t * t, dt)  # beta = 0: the output window itself is poison
    flags = (4 if fc else 0) | (VB if dt == BF16 else 0)
    disp = (dt, t, t, t, t, t, t, t * t, t * t, flags)
    ep = (0, 5, 4, 1) if fc else (0, 0, 0, 0)
    old = (rt.set_vnni_factor(vn), orc.set_vnni_factor(vn)) if dt == BF16 else None
    old_async, old_q = rt.set_async(True), rt.set_tile_queue(1)
    names = []
    try:
        h = rt.fused_brgemm_dispatch(*disp, *ep)
        dA, dW, dB, dC = dev(A), dev(W), dev(bias), dev(C0)
        ref = C0.copy()
        for p in range(passes):
            for i in range(MB):
                for j in range(NB):
                    args = (A, i * KB * t * t, W, j * KB * t * t, ref, (i * NB + j) * t * t, bias, j * t, KB)
                    orc.fused_brgemm(*disp, *ep, *args)
                    rt.fused_brgemm(dt, h, dA, i * KB * t * t, dW, j * KB * t * t, dC, (i * NB + j) * t * t, dB, j * t, KB)
            rt.synchronize()
            names.append(rt.last_grouped_kernel())
            got = host(dC, C0)
            ed.check_bits(got[:MB * NB * t * t], ref[:MB * NB * t * t], dt, "queued layer pass %d [%s]" % (p, names[-1]))
            assert np.array_equal(ed.bits(got[MB * NB * t * t:]), ed.bits(C0[MB * NB * t * t:])), "wrote past the output"
    finally:
        rt.synchronize()
        rt.set_tile_queue(old_q)
        rt.set_async(old_async)
        if old:
            rt.set_vnni_factor(old[0])
            orc.set_vnni_factor(old[1])
    assert any(expect in nm for nm in names), (expect, names)
    return names


@pytest.mark.parametrize("fc", [False, True], ids=["matmul_beta1", "fc_beta0_bias_relu"])
def test_exact_tile_queue_f32_groups(rt, fc):
    for nm in _queue_layer(rt, F32, 128, 256, 256, 32, 2, fc, 2, "grouped"):
        seen("grouped", nm)


@pytest.mark.parametrize("vn", [2, 4])
@pytest.mark.parametrize("fc", [False, True], ids=["matmul_beta1", "fc_beta0_bias_relu"])
def test_exact_tile_queue_bf16_groups_and_quads(rt, vn, fc):
    names = _queue_layer(rt, BF16, 512, 2560, 128, 64, vn, fc, 3, "quads")
    for nm in names:
        seen("quads" if "quads" in nm else "grouped", nm)


@pytest.mark.parametrize("fused", [False, True])
def test_exact_merged_tile_grid(rt, fused):
    """tile invokes over ONE flat problem (A by tile row, B by tile column, C by both): replays run as one merged launch, bit-exact"""
    rng = np.random.default_rng(31 + fused)
    M, N, K, tm, tn = 256, 256, 128, 32, 64
    br = 2 if fused else 1
    k = K // br
    ra, rb, rc = ed.exact_ranges(F32, K)
    X, W, bias = ed.exact_fill(rng, M * K, F32, ra), ed.exact_fill(rng, K * N, F32, rb), ed.exact_fill(rng, N, F32, rc)
    C0 = ed.exact_fill(rng, M * N, F32, rc)
    ep = (0, 5, 4, 1) if fused else (0, 0, 0, 0)
    disp = (F32, tm, tn, k, K, N, N, k, k * N, 4)
    h = rt.fused_brgemm_dispatch(*disp, *ep)
    grid = [(i, j) for i in range(M // tm) for j in range(N // tn)]
    ref = C0.copy()
    for (i, j) in grid:
        orc.fused_brgemm(*disp, *ep, X, i * tm * K, W, j * tn, ref, i * tm * N + j * tn, bias, j * tn, br)
    dX, dW, dB = dev(X), dev(W), dev(bias)
    old_async, old_q = rt.set_async(True), rt.set_tile_queue(1)
    names = []
    try:
        dOut = dev(C0)
        for rep in range(3):
            dOut.copy_(dev(np.full(M * N, np.nan, np.float32)))
            for (i, j) in grid:
                rt.fused_brgemm(F32, h, dX, i * tm * K, dW, j * tn, dOut, i * tm * N + j * tn, dB, j * tn, br)
            rt.synchronize()
            names.append(rt.last_grouped_kernel())
            ed.check_bits(host(dOut, ref), ref, F32, "grid pass %d [%s]" % (rep, names[-1]))
    finally:
        rt.set_tile_queue(old_q)
        rt.set_async(old_async)
    assert "merged" in names[-1], names
    seen("merged", names[-1])


# ---------------------------------------------------------------- chains
def _sparse_signs(rng, n, k):
    """weights in {-1, 0, 1}, about 4 nonzeros per column of k: integer activations stay integers and small at every layer"""
    q = min(1.0, 4.0 / k)
    return rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=n, p=[q / 2, 1 - q, q / 2])


def _check_chain_layers(dt, ch, x, got_layers, oracle_layer):
    """every layer bit for bit against the oracle fed the ORACLE's previous activations (exact data: the GPU's are the same bits),
    and the exactness precondition checked per layer: the oracle's output is the fp64 result rounded once"""
    prev = x
    for l in range(ch.L):
        k, n, ldi, ld = ch.dims[l], ch.dims[l + 1], ch.ld[l], ch.ld[l + 1]
        ref = oracle_layer(l, prev)
        sel = (np.arange(ch.m)[:, None] * ld + np.arange(n)[None, :]).reshape(-1)
        xin = ed.as_f32(prev).reshape(ch.m, ldi)[:, :k].astype(np.float64)
        w = ed.as_f32(ch.W[l]).astype(np.float64)
        w = w.reshape(k // 2, n, 2).transpose(0, 2, 1).reshape(k, n) if dt == BF16 else w.reshape(k, n)
        f64 = xin @ w + (ed.as_f32(ch.b[l]).astype(np.float64)[None, :] if ch.bias else 0)
        f64 = np.maximum(f64, 0) if ch.relu else f64
        assert np.array_equal(ed.bits(ed.store(f64.astype(np.float32).reshape(-1), dt)), ed.bits(ref[sel])), "layer %d not exact" % l
        ed.check_bits(got_layers[l][sel], ref[sel], dt, "chain layer %d" % l)
        prev = ref


@pytest.mark.parametrize("variant,m,dims", [(20, 128, [512, 512, 512]), (21, 128, [128, 256, 256]), (22, 128, [256, 256, 256, 256]),
                                            (23, 256, [256, 256, 256])], ids=lambda v: str(v).replace(" ", ""))
def test_exact_bf16_chain(rt, variant, m, dims):
    """the bf16 chain on exact data, bit-exact per layer; the input activation's padding columns are NaN"""
    from test_chain_gpu import Chain
    ch = Chain(rt, m, dims, seed=variant, force=variant, pad=8)
    rng = np.random.default_rng(variant)
    ch.W = [orc.f32_to_bf16(_sparse_signs(rng, dims[l] * dims[l + 1], dims[l])) for l in range(ch.L)]
    ch.b = [orc.f32_to_bf16(rng.integers(-40, 41, dims[l + 1]).astype(np.float32)) for l in range(ch.L)]
    ch.dW, ch.db = [dev(w) for w in ch.W], [dev(b) for b in ch.b]
    x = np.full(m * ch.ld[0], ed.BF16_NAN, np.uint16)
    x.reshape(m, ch.ld[0])[:, :dims[0]] = orc.f32_to_bf16(rng.integers(-15, 16, m * dims[0]).astype(np.float32)).reshape(m, -1)
    dacts = [dev(np.full(m * ch.ld[l + 1], ed.BF16_NAN, np.uint16)) for l in range(ch.L)]
    was_async = rt.set_async(True)
    try:
        assert rt.fused_brgemm_chain(BF16, ch.calls(dev(x), dacts)), "the chain did not run as one launch"
        rt.synchronize()
    finally:
        rt.set_async(was_async)
    seen("chain_bf16", rt.kernel_name(ch.handles[0]))

    def oracle_layer(l, prev):
        out = np.full(m * ch.ld[l + 1], ed.BF16_NAN, np.uint16)
        orc.fused_brgemm(BF16, m, dims[l + 1], 64, ch.ld[l], dims[l + 1], ch.ld[l + 1], 64, 64 * dims[l + 1], 4 | VB, 0, 5, 4, 1, prev, 0,
                         ch.W[l], 0, out, 0, ch.b[l], 0, dims[l] // 64)
        return out
    _check_chain_layers(BF16, ch, x, [host(d, x) for d in dacts], oracle_layer)


@pytest.mark.parametrize("variant,m,dims", [(7, 128, [256, 256, 256]), (6, 128, [128, 256, 256, 256])],
                         ids=lambda v: str(v).replace(" ", ""))
def test_exact_f32_chain(rt, variant, m, dims):
    """the f32 chain on exact data, bit-exact per layer; the input activation's padding columns are NaN, +inf, -inf"""
    from test_chain_f32_gpu import Chain32
    ch = Chain32(rt, m, dims, seed=variant, force=variant, pad=8)
    rng = np.random.default_rng(variant)
    ch.W = [_sparse_signs(rng, dims[l] * dims[l + 1], dims[l]) for l in range(ch.L)]
    ch.b = [rng.integers(-40, 41, dims[l + 1]).astype(np.float32) for l in range(ch.L)]
    ch.dW, ch.db = [dev(w) for w in ch.W], [dev(b) for b in ch.b]
    x = ed.poison_fill(m * ch.ld[0], F32)
    x.reshape(m, ch.ld[0])[:, :dims[0]] = rng.integers(-255, 256, (m, dims[0])).astype(np.float32)
    dacts = [dev(np.full(m * ch.ld[l + 1], np.nan, np.float32)) for l in range(ch.L)]
    was_async = rt.set_async(True)
    try:
        assert rt.fused_brgemm_chain(F32, ch.calls(dev(x), dacts)), "the chain did not run as one launch"
        rt.synchronize()
    finally:
        rt.set_async(was_async)
    seen("chain_f32", rt.kernel_name(ch.handles[0]))

    def oracle_layer(l, prev):
        out = np.full(m * ch.ld[l + 1], np.nan, np.float32)
        ch.oracle_layer(l, prev, out)
        return out
    _check_chain_layers(F32, ch, x, [host(d, x) for d in dacts], oracle_layer)


# ---------------------------------------------------------------- eltwise on special values
def _special_vector(dt, n, rng):
    tiny = np.finfo(np.float32).tiny
    base = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, tiny / 4, -tiny / 8, tiny, 3.0e38, -3.0e38, 1e-40, 2.0 ** -133,
                     3.3895e38, 0.5, 7.0], np.float32)
    v = base[rng.integers(0, base.size, n)]
    return ed.store(v, dt)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_eltwise_special_values(rt, dt):
    """binary add / mul / sub / div and unary relu / identity / transpose on +-0, subnormals, +-inf, NaN, x/0, 0/0, inf/inf and
    bf16 results that round to inf: arithmetic results match the oracle's NaN positions and every other bit; identity, transpose and
    the VNNI-2 pack keep NaN payloads bit for bit"""
    rng = np.random.default_rng(dt)
    m, n = 48, 40
    L, R = _special_vector(dt, m * n, rng), _special_vector(dt, m * n, rng)
    for kind in (1, 2, 3, 4):
        ref = np.zeros(m * n, L.dtype)
        orc.binary(kind, dt, m, n, n, n, n, 0, L, 0, R, 0, ref, 0)
        h = rt.binary_dispatch(kind, dt, m, n, n, n, n, 0)
        dO = dev(np.zeros(m * n, L.dtype))
        rt.binary(dt, h, dev(L), 0, dev(R), 0, dO, 0)
        ed.check_bits(host(dO, L), ref, dt, "binary kind %d on special values" % kind, special=True)
        assert np.isnan(ed.as_f32(ref)).any() and np.isinf(ed.as_f32(ref)).any()
    # NaN payloads: moves keep every bit
    X = L.copy()
    if dt == BF16:
        X[::7] = 0x7fd5
        X[3::11] = 0xffc1
    else:
        X.view(np.uint32)[::7] = 0x7fc01234
        X.view(np.uint32)[3::11] = 0xffc00001
    for kind, args in ((1, (m, n, n, n, 0)), (29, (m, n, n, m, 0))):
        ref = np.zeros(m * n, X.dtype)
        orc.unary(kind, dt, *args, X, 0, ref, 0)
        h = rt.unary_dispatch(kind, dt, *args)
        dO = dev(np.zeros(m * n, X.dtype))
        rt.unary(dt, h, dev(X), 0, dO, 0)
        assert np.array_equal(ed.bits(host(dO, X)), ed.bits(ref)), "unary kind %d changed bits" % kind
    if dt == BF16:
        ref = np.zeros(m * n, X.dtype)
        orc.unary(28, dt, m, n, n, n, 0, X, 0, ref, 0)
        h = rt.unary_dispatch(28, dt, m, n, n, n, 0)
        dO = dev(np.zeros(m * n, X.dtype))
        rt.unary(dt, h, dev(X), 0, dO, 0)
        assert np.array_equal(ed.bits(host(dO, X)), ed.bits(ref)), "VNNI-2 pack changed bits"
    ref = np.zeros(m * n, X.dtype)
    orc.unary(5, dt, m, n, n, n, 0, L, 0, ref, 0)
    h = rt.unary_dispatch(5, dt, m, n, n, n, 0)
    dO = dev(np.zeros(m * n, X.dtype))
    rt.unary(dt, h, dev(L), 0, dO, 0)
    ed.check_bits(host(dO, L), ref, dt, "relu on special values", special=True)


def test_zz_coverage():
    """runs last: every variant 0 .. 31, the generic kernel, grouped and quad replays, the merged grid, split launches and both chains
    were reached by the cases above (kernel names as reported by the runtime)"""
    want = set(range(32)) - {8} | {"generic", "grouped", "quads", "merged", "split", "chain_bf16", "chain_f32"}
    for key in sorted(SEEN, key=str):
        print("[exact] %-10s %s" % (key, sorted(SEEN[key])))
    missing = want - set(SEEN)
    assert not missing, "not reached: %s" % sorted(missing, key=str)
