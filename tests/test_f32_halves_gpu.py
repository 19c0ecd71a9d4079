"""Halves (include/tpp_xsmm_abi.h xsmm_hip_set_f32_halves) on a real MI355X: a whole-layer f32 call on the 64x64 + K2 loader-wave tile
whose every tile runs as two independent 64x32 + K2 workgroups. The form must not change a bit: every case runs the same call under
mode 0 - the launch as it has always been, the reference here - and under mode 2 on the same device operands, and compares the two C
buffers bit for bit, row padding and a poisoned guard band included; xsmm_hip_f32_halves_stats proves which form ran. Operands are
N(0, 1) floats, so that any change in the order of additions shows. One case is also held against the oracle with the f32 bars.
Calls the form must leave alone - n or m not in whole 64x64 tiles, a forced split, a tile-queue group, a chain launch - leave the counter
where it is; an f32 chain step still equals its separate calls bit for bit when those calls run as halves.
Every case puts the mode back to what it was."""
import importlib

import numpy as np
import pytest

from oracle import pyoracle as orc
from test_chain_f32_gpu import Chain32
from test_parity_gpu import F32, check_close, dev

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
V_64x64K2 = 6   # the variant number of the 64x64 + K2 loader-wave tile (forced: small outputs are planned on smaller tiles)
GUARD = 256     # poisoned elements in front of and behind the C window (a multiple of 4: the window stays 16-byte aligned)


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def poison(size):
    """NaN, +inf, -inf in turn, every NaN with its own payload: a moved or rewritten guard element changes bits"""
    p = np.empty(size, np.uint32)
    i = np.arange(size, dtype=np.uint32)
    p[:] = 0x7FC00000 | (i & 0xFFFF)
    p[1::3] = 0x7F800000
    p[2::3] = 0xFF800000
    return p.view(np.float32)


class Layer:
    """one whole-layer call: A [m][k * br] row-major read in br batch elements of k columns, B [k * br][n]; pad: lda, ldb and ldc exceed
    the rows they hold and every operand starts at a non-zero element offset"""

    def __init__(self, rt, m, n, k, br, beta0=True, bias=False, relu=False, pad=False, force=V_64x64K2, seed=0):
        self.rt, self.m, self.n, self.k, self.br, self.beta0, self.bias, self.relu = rt, m, n, k, br, beta0, bias, relu
        K = k * br
        self.lda, self.ldb, self.ldc = (K + 8, n + 4, n + 12) if pad else (K, n, n)
        self.offs = (4, 8, 4, 4) if pad else (0, 0, 0, 0)
        self.sa, self.sb = k, k * self.ldb
        rng = np.random.default_rng(seed)
        self.A = rng.standard_normal(self.offs[0] + m * self.lda + 8).astype(np.float32)
        self.B = rng.standard_normal(self.offs[1] + K * self.ldb + 8).astype(np.float32)
        self.D = rng.standard_normal(self.offs[3] + n + 8).astype(np.float32)
        # C: guard band, the element offset, m rows of ldc (the row padding poisoned too), guard band
        self.c_off = GUARD + self.offs[2]
        self.C = poison(self.c_off + m * self.ldc + GUARD)
        self.win = (self.c_off + np.arange(m)[:, None] * self.ldc + np.arange(n)[None, :]).reshape(-1)
        self.C[self.win] = rng.standard_normal(m * n).astype(np.float32)
        self.fused = bias or relu
        self.flags = 4 if beta0 else 0
        if force is not None:
            rt.force_variant(force)
        try:
            if self.fused:
                self.h = rt.fused_brgemm_dispatch(F32, m, n, k, self.lda, self.ldb, self.ldc, self.sa, self.sb, self.flags, 0, 5 if relu else 0,
                                                  4 if bias else 0, 1 if bias else 0)
            else:
                self.h = rt.brgemm_dispatch(F32, m, n, k, self.lda, self.ldb, self.ldc, self.sa, self.sb, self.flags)
        finally:
            if force is not None:
                rt.force_variant(-1)
        self.dA, self.dB, self.dD = dev(self.A), dev(self.B), dev(self.D)

    def run(self, mode):
        """the call under `mode` on a fresh copy of C; returns (all of C's bits, the counters' movement, the refined kernel text)"""
        rt = self.rt
        dC = dev(self.C)
        before = rt.f32_halves_stats()
        prev = rt.set_f32_halves(mode)
        assert prev >= 0
        try:
            if self.fused:
                rt.fused_brgemm(F32, self.h, self.dA, self.offs[0], self.dB, self.offs[1], dC, self.c_off, self.dD, self.offs[3], self.br)
            else:
                rt.brgemm(F32, self.h, self.dA, self.offs[0], self.dB, self.offs[1], dC, self.c_off, self.br)
            rt.synchronize()
            refined = rt.last_refined_kernel()
        finally:
            rt.set_f32_halves(prev)
        after = rt.f32_halves_stats()
        return dC.cpu().numpy().view(np.uint32), (after[0] - before[0], after[1], after[2]), refined

    def both(self, eligible=True):
        """mode 0, then mode 2: the same bits everywhere; the counter moves under mode 2 only, and only for an eligible call"""
        what = "m%d n%d k%d br%d beta0=%d bias=%d relu=%d lda%d ldb%d ldc%d [%s]" % (
            self.m, self.n, self.k, self.br, self.beta0, self.bias, self.relu, self.lda, self.ldb, self.ldc, self.rt.kernel_name(self.h))
        plain, moved0, refined0 = self.run(0)
        halves, moved2, refined2 = self.run(2)
        assert moved0[0] == 0, what + ": the counter moved with the mode off"
        if eligible:
            assert "64x64,k2" in self.rt.kernel_name(self.h), what
            assert moved2 == (1, self.m // 64, self.n // 64), (what, moved2)
            assert refined0 == refined2 == "", (what, refined0, refined2)
        else:
            assert moved2[0] == 0, what + ": an ineligible call ran as halves"
            assert refined0 == refined2, (what, refined0, refined2)
        differ = plain != halves
        assert not differ.any(), "%s: %d elements differ between the two forms, the first at %d (window starts at %d)" % (
            what, int(differ.sum()), int(np.flatnonzero(differ)[0]), self.c_off)
        outside = np.ones(self.C.size, bool)
        outside[self.win] = False
        assert np.array_equal(halves[outside], self.C.view(np.uint32)[outside]), what + ": wrote outside the output window"
        return halves.view(np.float32)


# the smallest shapes at which the form can go wrong
CASES = [
    # one tile, two halves, fewer chunks than ring slots
    dict(m=64, n=64, k=64, br=1), dict(m=64, n=64, k=64, br=2),
    # around the 3-slot lap logic (the steady lap, the last lap of 1, 2 and 3 chunks)
    dict(m=128, n=192, k=64, br=3), dict(m=128, n=192, k=64, br=4), dict(m=128, n=192, k=64, br=5), dict(m=128, n=192, k=64, br=7),
    # two chunks per batch element
    dict(m=128, n=128, k=128, br=3),
    # lda > k, ldb > n, ldc > n, non-zero element offsets
    dict(m=64, n=128, k=64, br=4, pad=True),
    # beta = 1, and the fused bias + relu dispatch (beta 0 and beta 1)
    dict(m=64, n=128, k=64, br=4, beta0=False), dict(m=64, n=128, k=64, br=4, bias=True, relu=True),
    dict(m=64, n=128, k=64, br=4, beta0=False, bias=True, relu=True, pad=True),
    # tile counts the 8 XCD blocks do not divide
    dict(m=192, n=64, k=64, br=2),
    # more halves than two per CU: 272 tiles = 544 workgroups, a second round
    dict(m=1088, n=1024, k=64, br=2),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join("%s%s" % (k, int(v)) for k, v in c.items()))
def test_halves_give_the_bits_of_the_plain_launch(rt, case):
    Layer(rt, seed=sum(case.values()), **case).both()


def test_one_case_against_the_oracle(rt):
    """beta = 1, bias, relu, five chunks: the f32 bars of the suite (test_parity_gpu.check_close, element-wise criterion included)"""
    L = Layer(rt, 128, 192, 64, 5, beta0=False, bias=True, relu=True, pad=True, seed=77)
    got = L.both()
    ref, mag = L.C.copy(), L.C.copy()
    mag[L.win] = np.abs(mag[L.win])
    args = (F32, L.m, L.n, L.k, L.lda, L.ldb, L.ldc, L.sa, L.sb, L.flags, 0)
    orc.fused_brgemm(*args, 5, 4, 1, L.A, L.offs[0], L.B, L.offs[1], ref, L.c_off, L.D, L.offs[3], L.br)
    orc.fused_brgemm(*args, 0, 4, 1, np.abs(L.A), L.offs[0], np.abs(L.B), L.offs[1], mag, L.c_off, np.abs(L.D), L.offs[3], L.br)
    check_close(got[L.win], ref[L.win], F32, "halves against the oracle", mag[L.win], L.k * L.br)


@pytest.mark.parametrize("m,n", [(64, 96), (96, 64)])
def test_a_shape_not_in_whole_tiles_is_left_alone(rt, m, n):
    Layer(rt, m, n, 64, 4, seed=m + n).both(eligible=False)   # (the forced tile does not divide the shape: another kernel runs)
    Layer(rt, m, n, 64, 4, force=None, seed=m).both(eligible=False)


def test_a_forced_split_is_left_alone(rt):
    L = Layer(rt, 64, 128, 64, 4, seed=3)   # (four chunks: the split model leaves the call alone, a forced count of 2 takes it)
    prev = rt.force_split(2)
    try:
        L.both(eligible=False)
        assert rt.last_refined_kernel().endswith(", split"), rt.last_refined_kernel()
    finally:
        rt.force_split(prev)
    L.both()   # and without the forced count the same call is taken


def test_a_tile_queue_group_is_left_alone(rt):
    """64x64x64 items through the tile queue: what the queue groups is planned by plan_gemm_group, which knows no halves"""
    tm = tn = tk = 64
    MB, NB, KB = 4, 6, 2
    rng = np.random.default_rng(8)
    X = rng.standard_normal(MB * KB * tm * tk).astype(np.float32)
    W = rng.standard_normal(NB * KB * tk * tn).astype(np.float32)
    C0 = rng.standard_normal(MB * NB * tm * tn).astype(np.float32)
    h = rt.brgemm_dispatch(F32, tm, tn, tk, tk, tn, tn, tm * tk, tk * tn, 0)
    dX, dW = dev(X), dev(W)
    before = rt.f32_halves_stats()
    prev_async, prev_q, prev_mode = rt.set_async(True), rt.set_tile_queue(1), rt.set_f32_halves(0)
    results = {}
    try:
        for mode in (0, 2):
            rt.set_f32_halves(mode)
            for rep in range(3):  # recorded, then replayed
                dC = dev(C0)
                rt.synchronize()
                for i in range(MB):
                    for j in range(NB):
                        rt.brgemm(F32, h, dX, i * KB * tm * tk, dW, j * KB * tk * tn, dC, (i * NB + j) * tm * tn, KB)
                rt.synchronize()
                results[(mode, rep)] = (rt.last_grouped_kernel(), dC.cpu().numpy().view(np.uint32).tobytes())
    finally:
        rt.set_f32_halves(prev_mode)
        rt.synchronize()
        rt.set_tile_queue(prev_q)
        rt.set_async(prev_async)
    assert results[(0, 2)][0] != "", "the items were not grouped"
    for rep in range(3):
        assert results[(2, rep)] == results[(0, rep)], rep
    assert rt.f32_halves_stats() == before


def test_a_chain_is_left_alone_and_equals_its_calls_run_as_halves(rt):
    """three 64x64 + K2 layers: the chain launch does not count as halves, its separate calls under mode 2 do, the bits are the same"""
    import torch
    ch = Chain32(rt, 128, [128, 256, 256, 256], seed=31, force=V_64x64K2)
    start = [np.full(ch.m * ch.ld[l + 1], np.nan, np.float32) for l in range(ch.L)]
    dacts_f, dacts_s = [dev(a) for a in start], [dev(a) for a in start]
    was_async = rt.set_async(True)
    prev_mode = rt.set_f32_halves(2)
    try:
        for step in range(2):
            dx = dev(ch.new_input())
            s0 = rt.f32_halves_stats()
            fused = rt.fused_brgemm_chain(F32, ch.calls(dx, dacts_f))
            rt.synchronize()
            assert fused, "the chain did not run as one launch"
            s1 = rt.f32_halves_stats()
            assert s1 == s0, "a chain launch counted as halves"
            for c in ch.calls(dx, dacts_s):
                rt.fused_brgemm(F32, *c)
            rt.synchronize()
            assert rt.f32_halves_stats()[0] == s1[0] + ch.L, "the separate calls did not run as halves"
            for l in range(ch.L):
                assert torch.equal(dacts_f[l].view(torch.int32), dacts_s[l].view(torch.int32)), "step %d layer %d" % (step, l)
                assert not torch.isnan(dacts_f[l]).any()
    finally:
        rt.synchronize()
        rt.set_f32_halves(prev_mode)
        rt.set_async(was_async)
