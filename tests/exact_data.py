"""Test data on which every correct GEMM kernel gives the oracle's bits, and the memory around it.

Exact inputs: operands are small integers times a power of two (A on 2^s, B on 2^t, C and bias on 2^(s+t)), and for every output
|C| + |bias| + sum_k |a||b| < 2^24 * 2^(s+t). Every product and every partial sum, in any order, is then an f32 number: a kernel's
accumulator equals the oracle's whatever its tiling, K split, split-launch count, queue grouping or chain seam, and the stored result
must match bit for bit - f32 as it is, bf16 after the one round-to-nearest-even store. Integer sums land on bf16 ties often
(257 lies halfway between 256 and 258), so truncation, rounding half away from zero and double rounding show up as bit differences.

Poison: every element of an operand buffer that a descriptor does not name (lda / ldb padding, gaps between batch elements, guard
tails, the whole C window under beta = 0) holds NaN or an infinity, so a kernel that reads it - even to multiply it by a zero pad -
corrupts the output."""
import math

import numpy as np

from oracle import pyoracle as orc

F32, BF16 = 1, 2
BF16_NAN, BF16_INF, BF16_NINF = 0x7fc0, 0x7f80, 0xff80


def utype(dt):
    return np.uint32 if dt == F32 else np.uint16


def bits(a):
    """the raw bit patterns of an f32 or bf16 (uint16) array"""
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint16)


def as_f32(a):
    return a if a.dtype == np.float32 else orc.bf16_to_f32(a)


def store(v, dt):
    v = np.asarray(v, dtype=np.float32)
    return v if dt == F32 else orc.f32_to_bf16(v)


def exact_ranges(dt, K, ra=None, rb=None):
    """integer ranges (Ra, Rb, Rc) of A, B and C / bias for K products per output, with K Ra Rb + 2 Rc (1 + 2^-8) < 2^24.
    bf16 draws stay small so that the sums fall where bf16 ties are frequent (a few hundred to a few thousand)."""
    K = max(int(K), 1)
    cap = 255 if dt == F32 else 15
    r = max(1, min(cap, math.isqrt((1 << 22) // K)))
    ra, rb = ra or r, rb or r
    rc = max(1, min(1 << 21, K * ra * rb // (4 if dt == F32 else 8)))
    assert K * ra * rb + 2 * rc * (1 + 2.0 ** -8) < 2 ** 24, (K, ra, rb, rc)
    return ra, rb, rc


def exact_fill(rng, n, dt, R, e=0):
    """n integers uniform in [-R, R] times 2^e, stored in dt (bf16: integers beyond 256 are rounded to the bf16 grid - still
    integers, at most 2^-8 larger)"""
    v = np.ldexp(rng.integers(-R, R + 1, n).astype(np.float64), e).astype(np.float32)
    return store(v, dt)


def poison_fill(n, dt, mixed=True):
    """NaN (bf16 0x7fc0); f32 buffers cycle NaN, +inf, -inf when `mixed`"""
    if dt == BF16:
        return np.full(n, BF16_NAN, np.uint16)
    p = np.full(n, np.nan, np.float32)
    if mixed:
        p[1::3] = np.inf
        p[2::3] = -np.inf
    return p


def b_live_index(kk, j, ldb, vnni, v):
    return (kk // v) * (v * ldb) + j * v + kk % v if vnni else kk * ldb + j


def c_live_index(i, j, ldc, vnni_c):
    return (i // 2) * (2 * ldc) + 2 * j + i % 2 if vnni_c else i * ldc + j


def live_masks(sizes, m, n, k, br, lda, ldb, ldc, sa, sb, offs, vnni=False, v=2, beta0=False, bias=False, vnni_c=False):
    """element masks of what the descriptor names in buffers of `sizes` = (nA, nB, nC, nD): A and B over the UNION of all batch
    windows (overlapping batches work), C's output footprint unless beta = 0, the bias row when there is one"""
    la, lb, lc, ld_ = (np.zeros(s, bool) for s in sizes)
    ii, kk, jj = np.arange(m)[:, None], np.arange(k)[None, :], np.arange(n)[None, :]
    for b in range(br):
        if m and k:
            la[offs[0] + b * sa + ii * lda + kk] = True
        if k and n:
            lb[offs[1] + b * sb + b_live_index(np.arange(k)[:, None], jj, ldb, vnni, v)] = True
    if not beta0 and m and n:
        lc[offs[2] + c_live_index(ii, jj, ldc, vnni_c)] = True
    if bias and n:
        ld_[offs[3] + np.arange(n)] = True
    return la, lb, lc, ld_


def sprinkle_special(rng, arr, live, dt, count):
    """put inf, -inf and NaN at `count` random live elements of `arr` (in place); returns the positions"""
    pos = np.flatnonzero(live)
    if not pos.size:
        return pos
    pos = rng.choice(pos, size=min(count, pos.size), replace=False)
    vals = np.array([np.inf, -np.inf, np.nan], np.float32)[np.arange(pos.size) % 3]
    arr[pos] = store(vals, dt)
    return pos


def check_bits(got, ref, dt, what, special=False):
    """bit-exact comparison; with `special`, non-finite results are compared by kind (NaN / +inf / -inf) and the finite ones bit
    for bit (NaN payloads and signs are not pinned)"""
    g, r = as_f32(got), as_f32(ref)
    if special:
        for f in (np.isnan, np.isposinf, np.isneginf):
            bad = f(g) != f(r)
            assert not bad.any(), "%s: %s differs at %d elements (first at %d: got %r, oracle %r)" % (
                what, f.__name__, int(bad.sum()), int(np.flatnonzero(bad)[0]), g[bad][0], r[bad][0])
        fin = np.isfinite(r)
        gb, rb = bits(got)[fin], bits(ref)[fin]
    else:
        assert np.isfinite(r).all(), what + ": the oracle's result is not finite - the live mask misses something it reads"
        gb, rb = bits(got), bits(ref)
    bad = gb != rb
    if bad.any():
        gf, rf = g[fin] if special else g, r[fin] if special else r
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d/%d elements differ in bits (first: got %r = 0x%x, oracle %r = 0x%x)" % (
            what, int(bad.sum()), bad.size, float(gf[i]), int(gb[i]), float(rf[i]), int(rb[i])))


# ---------------------------------------------------------------- targeted rounding cases (bf16 stores)
HALF_TO_INF = (2.0 - 2.0 ** -8) * 2.0 ** 127   # halfway between the largest finite bf16 (0x7f7f) and 2^128


def rounding_targets():
    """(acc, c) pairs of f32 numbers - acc the sum of products, c the beta = 1 input - whose totals are bf16 ties, near-ties,
    ordinary roundings at both signs, or sit at the overflow edge; the (acc, c) traps are ties only if acc were rounded first"""
    t = []
    for base in (256.0, 1024.0, 3.0 * 2 ** 10, 2.0 ** -20 * 384):
        ulp = 2.0 ** (math.floor(math.log2(base)) - 7)  # bf16 spacing at base
        for s in (1.0, -1.0):
            t.append((s * (base + ulp / 2), 0.0))               # tie, even neighbour below
            t.append((s * (base + 3 * ulp / 2), 0.0))           # tie, even neighbour above
            t.append((s * (base + ulp / 2 + ulp / 64), 0.0))    # just above a tie
            t.append((s * (base + ulp / 2 - ulp / 64), 0.0))    # just below a tie
            t.append((s * (base + ulp / 4), 0.0))               # ordinary rounding down
            t.append((s * (base + 3 * ulp / 4), 0.0))           # ordinary rounding up
    # C + acc is just off a tie, but rounding acc first (1 + 2^-9 -> 1, 3 - 2^-8 -> 3) would make it a tie
    for s in (1.0, -1.0):
        t.append((s * (1.0 + 2.0 ** -9), s * 256.0))
        t.append((s * (3.0 - 2.0 ** -8), s * 256.0))
        t.append((s * (4.0 + 2.0 ** -6), s * 1024.0))
    big = float(orc.bf16_to_f32(np.array([0x7f7f], np.uint16))[0])
    for s in (1.0, -1.0):
        t.append((s * big, 0.0))                             # the largest finite bf16 stays finite
        t.append((s * HALF_TO_INF, 0.0))                     # the halfway point to 2^128 rounds to inf
        t.append((s * (HALF_TO_INF + 2.0 ** 104), 0.0))      # above it
        t.append((s * (HALF_TO_INF - 2.0 ** 104), 0.0))      # one f32 ulp below it: stays finite
    return t


BIAS_ACC = [1.0 + 2.0 ** -9, 3.0 - 2.0 ** -8, -(1.0 + 2.0 ** -9), 2.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -10]


def split3(x):
    """x (f32 numbers) as hi + mid + lo, three bf16 numbers (truncated parts) whose partial sums in any order are f32 numbers"""
    x = np.ascontiguousarray(x, np.float32)
    hi = orc.bf16_to_f32(_trunc(x))
    r1 = (x - hi).astype(np.float32)
    mid = orc.bf16_to_f32(_trunc(r1))
    lo = (r1 - mid).astype(np.float32)
    assert np.array_equal(orc.bf16_to_f32(orc.f32_to_bf16(lo)), lo)
    assert np.array_equal((hi.astype(np.float64) + mid + lo).astype(np.float32), x)
    return hi, mid, lo


def _trunc(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def rounding_case(m, n, k):
    """flat bf16 operands (bits) A [m][k], B [k][n], C [m][n], bias [n] whose outputs run through rounding_targets(): row i selects
    group g = i mod (k // 3) - A's row holds ones at columns 3g, 3g + 1, 3g + 2 - and B's rows 3g .. 3g + 2 hold the three bf16 parts
    of the accumulator target of (g, j), so acc = hi + mid + lo exactly in any order. Every 8th column is a bias column: bias 256,
    c = 0, acc from BIAS_ACC (a tie only if acc were rounded before the bias is added). Returns A, B, C, D."""
    G = k // 3
    assert G >= 1
    tg = rounding_targets()
    acc = np.zeros((G, n), np.float32)
    cg = np.zeros((G, n), np.float32)
    bias = np.zeros(n, np.float32)
    for g in range(G):
        for j in range(n):
            if j % 8 == 7:
                acc[g, j], bias[j] = BIAS_ACC[(g * n + j) % len(BIAS_ACC)], 256.0
            else:
                acc[g, j], cg[g, j] = tg[(g * n + j) % len(tg)]
    A = np.zeros((m, k), np.float32)
    rows = np.arange(m) % G
    for p in range(3):
        A[np.arange(m), 3 * rows + p] = 1.0
    B = np.zeros((k, n), np.float32)
    for p, part in enumerate(split3(acc.reshape(-1))):
        B[3 * np.arange(G) + p, :] = part.reshape(G, n)
    C = cg[rows]
    return (orc.f32_to_bf16(A.reshape(-1)), orc.f32_to_bf16(B.reshape(-1)), orc.f32_to_bf16(C.reshape(-1)),
            orc.f32_to_bf16(bias))
