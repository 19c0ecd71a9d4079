"""Narrow-output f32 layers (xsmm_hip_set_narrow_f32) on a real MI355X, under the forcing modes: m in {32, 33, 47, 65, 200} (one block;
clamped rows in a single block and in a last block; several blocks), n in {1, 10, 16, 17, 31} (one accumulator set partly used, full, two
sets), (k, br) from one step with idle waves over masked lane groups and a ragged tail to more steps than waves, every BM. Operands are
strided - lda > k, ldb = n + 5, ldc = n + 3 (rows only 4-byte aligned), unpacked batch strides, C and the bias moved by an odd element
count -, NaN in every gap and guard row, a bit pattern around C that every run compares; every taken call asserts kernel and stats."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_data as ed  # noqa: E402
from test_skinny_f32_gpu import EPS, F32, KBR, Case  # noqa: E402

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
MS, NS, BMS = [32, 33, 47, 65, 200], [1, 10, 16, 17, 31], [16, 32, 64]


class NarrowCase(Case):
    """test_skinny_f32_gpu.Case with the layout this kernel is for: ldb = n + 5, ldc = n + 3, C moved by 9 and the bias by 5 elements, A by
    a_off (4: 16 bytes); lda, both batch strides, the poison and the bit pattern around C as there. rows_of: this problem holds that one's
    operands in its first rows (the same n, k and br, more rows)."""

    def __init__(self, m, n, k, br, seed, exact=False, lo=-3, beta0=True, bias=True, relu=True, a_off=4, rows_of=None):
        self.m, self.n, self.k, self.br, self.beta0, self.bias, self.relu = m, n, k, br, beta0, bias, relu
        self.lda, self.sa, self.ldb, self.ldc, self.o = br * (k + 4) + 4, k + 4, n + 5, n + 3, (a_off, 8, 9, 5)
        self.sb, o = (k + 3) * self.ldb, self.o
        sizes = (o[0] + (br - 1) * self.sa + m * self.lda + 4, o[1] + (br - 1) * self.sb + (k + 1) * self.ldb + 4, o[2] + m * self.ldc + 8, o[3] + n + 4)
        rng = np.random.default_rng(seed)
        draw = (lambda s: rng.integers(lo, 4, s).astype(np.float32)) if exact else (lambda s: rng.uniform(-1, 1, s).astype(np.float32))
        self.A, self.B, self.D = (np.full(s, np.nan, np.float32) for s in (sizes[0], sizes[1], sizes[3]))
        self.C = ((np.arange(sizes[2], dtype=np.uint32) * 2654435761 + 12345) & 0x7F7FFFFF).view(np.float32)  # the bit pattern around C
        self.ia, self.ib, self.ic = self.idx(m, n)
        self.A[self.ia], self.B[self.ib], self.C[self.ic], self.D[5:5 + n] = draw(self.ia.shape), draw(self.ib.shape), draw(self.ic.shape), draw(n)
        if rows_of is not None:
            s, (ja, jb, jc) = rows_of, self.idx(rows_of.m, n)
            self.A[ja], self.B[jb], self.C[jc], self.D[5:5 + n] = s.A[s.ia], s.B[s.ib], s.C[s.ic], s.D[5:5 + n]
        if beta0:
            self.C[self.ic] = np.nan
        if not bias:
            self.D[:] = np.nan

    def fp64(self):
        """(the result in fp64, sum |a b| + |c_in| + |bias| per element)"""
        a, b = self.A[self.ia].astype(np.float64), self.B[self.ib].astype(np.float64)
        c = np.zeros((self.m, self.n)) if self.beta0 else self.C[self.ic].astype(np.float64)
        d = self.D[5:5 + self.n].astype(np.float64)[None, :] if self.bias else 0.0
        acc = c + np.einsum("bik,bkj->ij", a, b) + d
        return (np.maximum(acc, 0) if self.relu else acc), np.einsum("bik,bkj->ij", np.abs(a), np.abs(b)) + np.abs(c) + np.abs(d)


@functools.lru_cache(maxsize=None)  # built once, shared by the three BM, never changed; the exact case's precondition asserted for every case
def cases(m, n, k, br, i):
    exact, rnd = NarrowCase(m, n, k, br, 31 * m + n + 10 * k + br + i, exact=True, **EPS[i]), NarrowCase(m, n, k, br, 77 * m + n + 10 * k + br + i, **EPS[i])
    want = exact.fp64()[0].astype(np.float32)
    assert np.array_equal(exact.oracle(), want), "precondition: the oracle is not the fp64 result"
    return exact, want, rnd, rnd.fp64()


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def mode_off(rt):
    rt.set_narrow_f32(0)
    yield
    rt.set_narrow_f32(0)


def run_taken(rt, case, bm):
    rt.set_narrow_f32(bm)
    before = rt.narrow_f32_stats()
    got, refined = case.run(rt)  # (asserts that nothing outside the m x n window changed)
    rt.set_narrow_f32(0)
    assert refined == "brgemm_f32_narrow<%dx%d>" % (bm, 16 if case.n <= 16 else 32), refined
    want = (before[0] + 1, -(-case.m // bm), min(8, case.br * -(-case.k // 16)), bm)
    assert rt.narrow_f32_stats() == want, (before, rt.narrow_f32_stats(), want)
    return got


def run_stays(rt, case, mode, **kw):
    rt.set_narrow_f32(mode)
    before = rt.narrow_f32_stats()
    got, refined = case.run(rt, **kw)[:2]
    assert "narrow" not in refined and rt.narrow_f32_stats() == before, refined
    return refined, got.tobytes()


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("bm", BMS)
def test_exact_bits_the_fp64_bound_three_runs_and_the_rows_of_a_taller_problem(rt, bm, k, br):
    for m, n, i in ((m, n, i) for m in MS for n in NS for i in range(len(EPS))):
        what = "bm%d m%d n%d k%d br%d beta0=%d" % (bm, m, n, k, br, EPS[i]["beta0"])
        exact, want, rnd, (ref, mag) = cases(m, n, k, br, i)
        # (a) integers in [-3, 3]: every partial sum is exact (9 br k <= 9000 < 2^24) - the fp64 result cast to f32, no tolerance
        ed.check_bits(run_taken(rt, exact, bm).reshape(-1), want.reshape(-1), F32, "exact " + what)
        # (b) random: |got - ref64| <= (br k + 3) 2^-24 (sum |a b| + |c_in| + |bias|), the worst case of any order of f32 accumulation;
        # three runs: finite, identical bits
        runs = [run_taken(rt, rnd, bm) for _ in range(3)]
        assert np.isfinite(runs[0]).all(), "read poisoned memory: " + what
        err, lim = np.abs(runs[0].astype(np.float64) - ref), (br * k + 3) * 2.0 ** -24 * mag
        print(what, "max err / bound %.3g" % (err / np.maximum(lim, 1e-300)).max())
        assert (err <= lim).all() and all(np.array_equal(r.view(np.uint32), runs[0].view(np.uint32)) for r in runs[1:]), what
        # placement: the bits of the same rows inside a taller problem on the same BM
        tall = run_taken(rt, NarrowCase(m + 2 * bm + 7, n, k, br, 1, rows_of=rnd, **EPS[i]), bm)
        ed.check_bits(runs[0].reshape(-1), tall[:m].reshape(-1), F32, "the rows of a taller problem: " + what)


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("bm", BMS)
def test_an_inf_counts_once(rt, bm, where):
    """k = 36: the last step keeps lane group 0 alone (k = 32 .. 35). Positive integers and one +Inf there: +Inf in exactly its row (A) or
    column (B), no NaN - a zero on one side only, or a load beyond k (NaN in the gaps), would give one"""
    for m, n in ((33, 10), (65, 31)):
        case, want = NarrowCase(m, n, 36, 1, m + bm, exact=True, lo=1), np.zeros((m, n), bool)
        if where == "A":
            case.A[case.ia[0, m - 1, 33]], want[m - 1, :] = np.inf, True
        else:
            case.B[case.ib[0, 33, n - 3]], want[:, n - 3] = np.inf, True
        got = run_taken(rt, case, bm)
        assert not np.isnan(got).any() and np.array_equal(np.isposinf(got), want) and not np.isneginf(got).any()


STAYS = [("n = 32", dict(n=32), {}), ("m = 31", dict(m=31), {}), ("k = 6", dict(k=6), {}), ("A off 16 bytes", dict(a_off=6), {}), ("a forced variant", {}, dict(force=8))]


@pytest.mark.parametrize("what,kw,run_kw", STAYS, ids=[s[0] for s in STAYS])
def test_calls_that_stay_under_mode_32(rt, what, kw, run_kw):
    case = NarrowCase(**{**dict(m=64, n=16, k=64, br=2, seed=5), **kw})
    assert run_stays(rt, case, 0, **run_kw) == run_stays(rt, case, 32, **run_kw), what
    run_taken(rt, NarrowCase(64, 16, 64, 2, 5), 32)  # (the eligible call these differ from IS taken)


def test_a_bf16_call_stays_under_mode_32(rt):
    from test_narrow_bf16_gpu import NarrowCase as Bf16Case
    assert run_stays(rt, Bf16Case(2, 64, 16, 64, 2, 5), 0) == run_stays(rt, Bf16Case(2, 64, 16, 64, 2, 5), 32)
    run_taken(rt, NarrowCase(64, 16, 64, 2, 5), 32)


def test_an_f32_mlp_with_a_10_wide_head_through_sharded_mlp(rt):
    """each layer against fp64 on the GPU's own input, within the bound of the random test (br k = the layer's k); the head alone is narrow"""
    import torch
    spec = pkg.MlpSpec(batch=40, layers=[64, 36, 10], dtype=F32)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (40, 64)).astype(np.float32)
    ws = [rng.uniform(-0.5, 0.5, (k, n)).astype(np.float32) for k, n in zip(spec.layers[:-1], spec.layers[1:])]
    bs = [rng.uniform(-1, 1, n).astype(np.float32) for n in spec.layers[1:]]
    dx, dw, db = torch.from_numpy(x).cuda(), [torch.from_numpy(w).cuda() for w in ws], [torch.from_numpy(b).cuda() for b in bs]
    for mode in (16, 0):
        rt.set_narrow_f32(mode)
        acts, before = [torch.full((40, n), float("nan"), device="cuda") for n in spec.layers[1:]], rt.narrow_f32_stats()[0]
        pkg.ShardedMlp(spec, rt=rt).forward(dx, dw, db, acts)
        torch.cuda.synchronize()
        assert rt.narrow_f32_stats()[0] == before + (1 if mode else 0)
        inp = x.astype(np.float64)
        for l, (w, b) in enumerate(zip(ws, bs)):
            got, w64 = acts[l].cpu().numpy(), w.astype(np.float64)
            err = np.abs(got - np.maximum(inp @ w64 + b, 0))
            assert (err <= (w.shape[0] + 3) * 2.0 ** -24 * (np.abs(inp) @ np.abs(w64) + np.abs(b))).all(), (mode, l, err.max())
            inp = got.astype(np.float64)
