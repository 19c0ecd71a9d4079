"""The test data of the bit-exact GPU suites (tests/exact_data.py), checked on the CPU oracle alone:
  * the exact-data generators meet their precondition - the oracle's f32 / bf16 result equals a float64 computation rounded once;
  * the bf16 cases hold many exact ties and ordinary roundings, and truncating, rounding half away from zero or rounding twice would
    change many output bits - so the GPU's bit-exact check can fail;
  * the live-mask builder is tight: poisoning any one sampled live element makes the oracle's output non-finite."""
import numpy as np
import pytest

import exact_data as ed
from oracle import pyoracle as orc

F32, BF16 = 1, 2
N_MIN = 50


def _flat_case(dt, m, n, k, br, beta0, bias, scale=(0, 0), seed=0):
    rng = np.random.default_rng(seed)
    ra, rb, rc = ed.exact_ranges(dt, k * br)
    s, t = scale
    A, B = ed.exact_fill(rng, m * k * br, dt, ra, s), ed.exact_fill(rng, k * br * n, dt, rb, t)
    C, D = ed.exact_fill(rng, m * n, dt, rc, s + t), ed.exact_fill(rng, n, dt, rc, s + t)
    return A, B, C, D


def _f64(A, B, C, D, m, n, K, beta0, bias, relu=False):
    """the exact result in float64 (A [m][K], B [K][n] flat)"""
    r = ed.as_f32(A).astype(np.float64).reshape(m, K) @ ed.as_f32(B).astype(np.float64).reshape(K, n)
    if not beta0:
        r += ed.as_f32(C).astype(np.float64).reshape(m, n)
    if bias:
        r += ed.as_f32(D).astype(np.float64)[None, :]
    return np.maximum(r, 0) if relu else r


def _oracle(dt, A, B, C, D, m, n, k, br, beta0, bias, relu=False):
    ref = C.copy()
    orc.fused_brgemm(dt, m, n, k, k * br, n, n, k, k * n, 4 if beta0 else 0, 0, 5 if relu else 0, 4 if bias else 0, 1 if bias else 0,
                     A, 0, B, 0, ref, 0, D, 0, br)
    return ref


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("k,br", [(64, 1), (64, 4), (64, 16), (64, 64)])
@pytest.mark.parametrize("scale", [(0, 0), (-60, -60), (50, 50), (-10, 4)])
def test_exact_generators_meet_their_precondition(dt, k, br, scale):
    m, n = 32, 48
    for beta0, bias, relu in ((False, True, False), (True, False, True)):
        A, B, C, D = _flat_case(dt, m, n, k, br, beta0, bias, scale, seed=k + br)
        ref = _oracle(dt, A, B, C, D, m, n, k, br, beta0, bias, relu)
        exact = _f64(A, B, C, D, m, n, k * br, beta0, bias, relu)
        # every partial sum is an f32 number: the f64 sum is one, and the oracle's f32 chain equals it rounded once
        assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
        assert np.array_equal(ed.bits(ref), ed.bits(ed.store(exact.astype(np.float32).reshape(-1), dt)))


def _roundings(acc, dt_bits):
    """bf16 of an f32 array in four ways: RNE (the store), truncation, half away from zero"""
    u = np.ascontiguousarray(acc, np.float32).view(np.uint32).astype(np.uint64)
    rne = orc.f32_to_bf16(acc)
    trunc = (u >> 16).astype(np.uint16)
    away = ((u + 0x8000) >> 16).astype(np.uint16)
    return rne, trunc, away


def test_bf16_random_exact_data_has_ties_and_catches_wrong_roundings():
    m, n, k, br = 128, 128, 64, 4
    A, B, C, D = _flat_case(BF16, m, n, k, br, False, True, seed=7)
    exact = _f64(A, B, C, D, m, n, k * br, False, True).astype(np.float32).reshape(-1)
    u = exact.view(np.uint32)
    low = u & 0xffff
    ties = int((low == 0x8000).sum())
    ordinary = int(((low != 0) & (low != 0x8000)).sum())
    assert ties >= N_MIN and ordinary >= N_MIN, (ties, ordinary)
    rne, trunc, away = _roundings(exact, True)
    ref = _oracle(BF16, A, B, C, D, m, n, k, br, False, True)
    assert np.array_equal(ref, rne)
    assert int((trunc != rne).sum()) >= N_MIN and int((away != rne).sum()) >= N_MIN
    # rounding twice: the bias / C added after the products' sum was rounded to bf16 on its own
    prod = _f64(A, B, C, D, m, n, k * br, True, False).astype(np.float32).reshape(-1)
    twice = orc.f32_to_bf16((ed.as_f32(orc.f32_to_bf16(prod)).astype(np.float64).reshape(m, n) + ed.as_f32(C).reshape(m, n)
                             + ed.as_f32(D)[None, :]).astype(np.float32).reshape(-1))
    assert int((twice != rne).sum()) >= N_MIN


@pytest.mark.parametrize("m,n", [(64, 96), (128, 192), (96, 72), (256, 256)])
def test_rounding_cases_hold_ties_traps_and_the_overflow_edge(m, n):
    k = 64
    A, B, C, D = ed.rounding_case(m, n, k)
    ref = _oracle(BF16, A, B, C, D, m, n, k, 1, False, True)
    Af, Bf = ed.as_f32(A).reshape(m, k).astype(np.float64), ed.as_f32(B).reshape(k, n).astype(np.float64)
    acc = Af @ Bf
    exact = acc + ed.as_f32(C).reshape(m, n) + ed.as_f32(D)[None, :]
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)  # totals are f32 numbers: one rounding, at the store
    e32 = exact.astype(np.float32).reshape(-1)
    rne, trunc, away = _roundings(e32, True)
    assert np.array_equal(ref, rne)
    low = e32.view(np.uint32) & 0xffff
    assert int((low == 0x8000).sum()) >= N_MIN and int(((low != 0) & (low != 0x8000)).sum()) >= N_MIN
    assert int((trunc != rne).sum()) >= N_MIN and int((away != rne).sum()) >= N_MIN
    # rounding acc before adding C and the bias changes bits
    twice = orc.f32_to_bf16((ed.as_f32(orc.f32_to_bf16(acc.astype(np.float32).reshape(-1))).reshape(m, n).astype(np.float64)
                             + ed.as_f32(C).reshape(m, n) + ed.as_f32(D)[None, :]).astype(np.float32).reshape(-1))
    assert int((twice != rne).sum()) >= 8
    b = ed.bits(ref)
    assert (b == 0x7f7f).any() and (b == 0xff7f).any() and (b == 0x7f80).any() and (b == 0xff80).any()
    # the element one f32 ulp below the halfway point to 2^128 stays finite, the halfway point itself does not
    assert (e32 == np.float32(ed.HALF_TO_INF - 2.0 ** 104)).any() and (e32 == np.float32(ed.HALF_TO_INF)).any()


@pytest.mark.parametrize("case", [
    # dt, m, n, k, br, lda, ldb, ldc, sa, sb, offs, vnni, v, beta0, bias, vnni_c
    (F32, 13, 17, 10, 3, 13, 19, 18, 13 * 13, 10 * 19, (1, 2, 3, 1), False, 2, False, True, False),
    (F32, 16, 24, 32, 4, 32 * 4 + 8, 28, 28, 32, 32 * 28, (4, 8, 4, 4), False, 2, True, True, False),
    (F32, 8, 8, 8, 6, 64, 16, 8, 8, 8, (0, 0, 0, 0), False, 2, False, False, False),   # overlapping batch elements
    (BF16, 12, 10, 8, 3, 10, 13, 12, 12 * 10, 8 * 13, (2, 2, 3, 1), True, 2, False, True, False),
    (BF16, 12, 10, 8, 2, 10, 13, 12, 12 * 10, 8 * 13, (2, 2, 3, 1), True, 4, False, True, False),
    (BF16, 6, 6, 6, 2, 8, 7, 9, 48, 42, (2, 2, 3, 1), True, 2, False, True, True),    # VNNI-C output
    (BF16, 9, 11, 7, 2, 9, 12, 11, 81, 84, (1, 1, 1, 1), False, 2, False, True, False),
])
def test_live_masks_are_tight(case):
    """poisoning one sampled live element of A, B, C (beta = 1) or the bias makes the oracle's result non-finite; poisoning every
    element outside the masks leaves it finite and unchanged"""
    dt, m, n, k, br, lda, ldb, ldc, sa, sb, offs, vnni, v, beta0, bias, vnni_c = case
    old = orc.set_vnni_factor(v)
    try:
        kp = -(-k // v) * v
        bmat = kp * ldb if vnni else k * ldb
        sizes = (offs[0] + (br - 1) * sa + m * lda + 8, offs[1] + (br - 1) * sb + bmat + 2 * ldb + 8, offs[2] + m * ldc + 2 * ldc + 8,
                 offs[3] + n + 8)
        rng = np.random.default_rng(sum(sizes))
        bufs = [ed.exact_fill(rng, s, dt, 7) for s in sizes]
        live = ed.live_masks(sizes, m, n, k, br, lda, ldb, ldc, sa, sb, offs, vnni=vnni, v=v, beta0=beta0, bias=bias, vnni_c=vnni_c)
        flags = (4 if beta0 else 0) | (2048 if vnni else 0) | (8192 if vnni_c else 0)
        win = (offs[2] + ed.c_live_index(np.arange(m)[:, None], np.arange(n)[None, :], ldc, vnni_c)).reshape(-1)

        def run(A, B, C, D):
            out = C.copy()
            orc.fused_brgemm(dt, m, n, k, lda, ldb, ldc, sa, sb, flags, 0, 0, 4 if bias else 0, 1 if bias else 0, A, offs[0], B, offs[1],
                             out, offs[2], D, offs[3], br)
            return out[win]
        clean = run(*bufs)
        assert np.isfinite(ed.as_f32(clean)).all()
        poisoned = [b.copy() for b in bufs]
        for p, lv in zip(poisoned, live):
            p[~lv] = ed.poison_fill(p.size, dt)[~lv]
        assert np.array_equal(ed.bits(run(*poisoned)), ed.bits(clean)), "the oracle reads an element outside the live masks"
        for which in range(4):
            pos = np.flatnonzero(live[which])
            if not pos.size:
                continue
            for p in rng.choice(pos, size=min(12, pos.size), replace=False):
                bad = [b.copy() for b in bufs]
                bad[which][p] = ed.poison_fill(1, dt, mixed=False)[0]
                assert not np.isfinite(ed.as_f32(run(*bad))).all(), "buffer %d element %d is marked live but not read" % (which, p)
    finally:
        orc.set_vnni_factor(old)
