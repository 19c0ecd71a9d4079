"""Skinny-batch f32 layers (xsmm_hip_set_skinny_f32) on a real MI355X, under the forcing modes: m in {1, 7, 16, 17, 31}, n in {BN, BN + 4,
200}, (k, br) from one step to a long ragged k. Operands are strided (lda > k, ldb > n, ldc > n, unpacked batch strides) with NaN in every
gap and guard row and a bit pattern around C that every run checks; every taken call asserts the reported kernel and the stats.
As a program: one call in a process of its own (the strict-mode child of the stays test)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_data as ed  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
F32 = 1
MS = [1, 7, 16, 17, 31]
KBR = [(16, 1), (4, 1), (36, 1), (32, 3), (32, 16), (1000, 1)]
EPS = (dict(beta0=True, bias=True, relu=True), dict(beta0=False, bias=False, relu=False))


class Case:
    """one whole-layer f32 call; exact: integers in [lo, 3], else uniform [-1, 1); everything the descriptor does not name is NaN"""

    def __init__(self, m, n, k, br, seed, exact=False, lo=-3, beta0=True, bias=True, relu=True, coff=4, corner_of=None):
        self.m, self.n, self.k, self.br, self.beta0, self.bias, self.relu = m, n, k, br, beta0, bias, relu
        self.lda, self.sa, self.ldb, self.ldc, self.o = br * (k + 4) + 4, k + 4, n + 4, n + 8, (4, 8, coff, 4)
        self.sb, o = (k + 3) * self.ldb, self.o
        sizes = (o[0] + (br - 1) * self.sa + m * self.lda + 4, o[1] + (br - 1) * self.sb + (k + 1) * self.ldb + 4, o[2] + m * self.ldc + 8, o[3] + n + 4)
        rng = np.random.default_rng(seed)
        draw = (lambda s: rng.integers(lo, 4, s).astype(np.float32)) if exact else (lambda s: rng.uniform(-1, 1, s).astype(np.float32))
        self.A, self.B, self.D = (np.full(s, np.nan, np.float32) for s in (sizes[0], sizes[1], sizes[3]))
        self.C = ((np.arange(sizes[2], dtype=np.uint32) * 2654435761 + 12345) & 0x7F7FFFFF).view(np.float32)  # the bit pattern around C
        self.ia, self.ib, self.ic = self.idx(m, n)
        self.A[self.ia], self.B[self.ib], self.C[self.ic], self.D[4:4 + n] = draw(self.ia.shape), draw(self.ib.shape), draw(self.ic.shape), draw(n)
        if corner_of is not None:  # this problem holds `corner_of` in its corner: the same k and br, more rows and columns
            s, (ja, jb, jc) = corner_of, self.idx(corner_of.m, corner_of.n)
            self.A[ja], self.B[jb], self.C[jc], self.D[4:4 + s.n] = s.A[s.ia], s.B[s.ib], s.C[s.ic], s.D[4:4 + s.n]
        if beta0:
            self.C[self.ic] = np.nan
        if not bias:
            self.D[:] = np.nan

    def idx(self, m, n):
        """element indices of A [br][m][k], B [br][k][n], C [m][n]"""
        b, kk, o = np.arange(self.br)[:, None, None], np.arange(self.k), self.o
        return (o[0] + b * self.sa + np.arange(m)[None, :, None] * self.lda + kk[None, None, :],
                o[1] + b * self.sb + kk[None, :, None] * self.ldb + np.arange(n)[None, None, :], o[2] + np.arange(m)[:, None] * self.ldc + np.arange(n)[None, :])

    def fp64(self):
        """(the result in fp64, sum |a b| + |c_in| + |bias| per element)"""
        a, b = self.A[self.ia].astype(np.float64), self.B[self.ib].astype(np.float64)
        c = np.zeros((self.m, self.n)) if self.beta0 else self.C[self.ic].astype(np.float64)
        d = self.D[4:4 + self.n].astype(np.float64)[None, :] if self.bias else 0.0
        acc = c + np.einsum("bik,bkj->ij", a, b) + d
        return (np.maximum(acc, 0) if self.relu else acc), np.einsum("bik,bkj->ij", np.abs(a), np.abs(b)) + np.abs(c) + np.abs(d)

    def args(self):
        return (F32, self.m, self.n, self.k, self.lda, self.ldb, self.ldc, self.sa, self.sb, 4 if self.beta0 else 0)

    def oracle(self):
        ref, o = self.C.copy(), self.o
        orc.fused_brgemm(*self.args(), 0, 5 if self.relu else 0, 4 if self.bias else 0, 1 if self.bias else 0, self.A, o[0], self.B, o[1], ref, o[2], self.D, o[3], self.br)
        return ref[self.ic]

    def run(self, rt, force=None):
        """on device copies: the m x n window after the call (everything around it checked), what xsmm_hip_last_refined_kernel reported"""
        import torch
        fused, o = self.bias or self.relu, self.o
        rt.force_variant(-1 if force is None else force)
        h = (rt.fused_brgemm_dispatch(*self.args(), 0, 5 if self.relu else 0, 4 if self.bias else 0, 1 if self.bias else 0) if fused else rt.brgemm_dispatch(*self.args()))
        rt.force_variant(-1)
        dA, dB, dC, dD = (torch.from_numpy(x.copy()).cuda() for x in (self.A, self.B, self.C, self.D))
        if fused:
            rt.fused_brgemm(F32, h, dA, o[0], dB, o[1], dC, o[2], dD, o[3], self.br)
        else:
            rt.brgemm(F32, h, dA, o[0], dB, o[1], dC, o[2], self.br)
        got, outside = dC.cpu().numpy(), np.ones(self.C.size, bool)
        outside[self.ic] = False
        assert np.array_equal(got[outside].view(np.uint32), self.C[outside].view(np.uint32)), "wrote outside the m x n window"
        return got[self.ic], rt.last_refined_kernel()


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def mode_off(rt):
    rt.set_skinny_f32(0)
    yield
    rt.set_skinny_f32(0)


def run_taken(rt, case, bn):
    rt.set_skinny_f32(bn)
    before = rt.skinny_f32_stats()
    got, refined = case.run(rt)
    rt.set_skinny_f32(0)
    assert refined == "brgemm_f32_skinny<%dx%d>" % (16 if case.m <= 16 else 32, bn), refined
    assert rt.skinny_f32_stats() == (before[0] + 1, -(-case.n // bn), min(8, case.br * -(-case.k // 16)), bn), (before, rt.skinny_f32_stats())
    return got


def run_stays(rt, case, mode, force=None):
    rt.set_skinny_f32(mode)
    before = rt.skinny_f32_stats()
    got, refined = case.run(rt, force)[:2]
    assert "f32_skinny" not in refined and rt.skinny_f32_stats() == before, refined
    return refined, got.tobytes()


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("bn", [16, 32, 64])
def test_exact_bits_the_fp64_bound_three_runs_and_the_corner_of_a_larger_problem(rt, bn, k, br):
    for m, n, (i, ep) in ((m, n, e) for m in MS for n in (bn, bn + 4, 200) for e in enumerate(EPS)):
        what = "m%d n%d k%d br%d bn%d beta0=%d" % (m, n, k, br, bn, ep["beta0"])
        # 1. integers in [-3, 3]: every partial sum is exact (9 br k <= 9000 < 2^24) - the fp64 result cast to f32, no tolerance
        case = Case(m, n, k, br, 31 * m + n + 10 * k + br + i, exact=True, **ep)
        want = case.fp64()[0].astype(np.float32)
        assert np.array_equal(case.oracle(), want), "precondition: the oracle is not the fp64 result"
        ed.check_bits(run_taken(rt, case, bn).reshape(-1), want.reshape(-1), F32, "exact " + what)
        # 2. random: |got - ref64| <= (br k + 3) 2^-24 (sum |a b| + |c_in| + |bias|), the worst case of any order of f32 accumulation, fused
        # or not; three runs on NaN-refilled outputs: finite, identical bits
        case = Case(m, n, k, br, 77 * m + n + 10 * k + br + i, **ep)
        runs, (ref, mag) = [run_taken(rt, case, bn) for _ in range(3)], case.fp64()
        assert np.isfinite(runs[0]).all(), "read poisoned memory: " + what
        err, lim = np.abs(runs[0].astype(np.float64) - ref), (br * k + 3) * 2.0 ** -24 * mag
        print(what, "max err / bound %.3g" % (err / np.maximum(lim, 1e-300)).max())
        assert (err <= lim).all() and all(np.array_equal(r.view(np.uint32), runs[0].view(np.uint32)) for r in runs[1:]), what
        # 3. placement: the bits of the same elements of a larger problem on the same BN that holds the call in its corner
        big = run_taken(rt, Case(16 if m <= 16 else 31, n + 2 * bn + 4, k, br, 1, corner_of=case, **ep), bn)
        ed.check_bits(runs[0].reshape(-1), big[:m, :n].reshape(-1), F32, "the corner of a larger problem: " + what)


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("bn", [16, 32, 64])
def test_an_inf_counts_once(rt, bn, where):
    """k = 36: the last step keeps lane group 0 alone (k = 32 .. 35). Positive integers and one +Inf there: +Inf in exactly its row (A) or
    column (B), no NaN - a zero on one side only, or a load beyond k (NaN in the gaps), would give one"""
    for m in (7, 31):
        n = bn + 4
        case, want = Case(m, n, 36, 1, m + bn, exact=True, lo=1), np.zeros((m, n), bool)
        if where == "A":
            case.A[case.ia[0, m - 1, 33]], want[m - 1, :] = np.inf, True
        else:
            case.B[case.ib[0, 33, n - 3]], want[:, n - 3] = np.inf, True
        got = run_taken(rt, case, bn)
        assert not np.isnan(got).any() and np.array_equal(np.isposinf(got), want) and not np.isneginf(got).any()


STAYS = [("m = 32", dict(m=32), None), ("k = 6", dict(k=6), None), ("an unaligned C", dict(coff=5), None), ("a forced generic kernel", {}, 8)]


@pytest.mark.parametrize("what,kw,force", STAYS, ids=[s[0] for s in STAYS])
def test_calls_that_stay_under_mode_64(rt, what, kw, force):
    case = Case(**{**dict(m=16, n=200, k=64, br=2, seed=5), **kw})
    assert run_stays(rt, case, 0, force) == run_stays(rt, case, 64, force), what
    run_taken(rt, Case(16, 200, 64, 2, 5), 64)  # (the eligible call these differ from IS taken)


def test_a_bf16_call_and_a_strict_mode_group_of_one_stay_under_mode_64(rt):
    from skinny_bf16_worker import Case as Bf16Case
    assert run_stays(rt, Bf16Case(2, 16, 200, 64, 2, 5), 0) == run_stays(rt, Bf16Case(2, 16, 200, 64, 2, 5), 64)
    out = {}  # strict mode is chosen before the first invoke: a child process each. m, n <= 64 runs as a tile-queue group of one
    for mode in ("0", "64"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}
        env.update(TPP_HIP_SKINNY_F32=mode, TPP_HIP_STRICT="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "16", "64", "64", "2", "9"], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        out[mode] = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["64"].pop("from_env") == 64 and out["0"].pop("from_env") == 0
    assert out["0"] == out["64"] and out["0"]["stats"] == [0, 0, 0, 0] and out["0"]["strict"] == 1, out


def test_a_batch_8_f32_mlp_through_sharded_mlp(rt):
    """each layer against fp64 on the GPU's own input, within the bound of the random test (br k = the layer's k); one launch per layer"""
    import torch
    spec = pkg.MlpSpec(batch=8, layers=[256, 200, 256, 64], dtype=F32)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (8, 256)).astype(np.float32)
    ws = [rng.uniform(-0.5, 0.5, (k, n)).astype(np.float32) for k, n in zip(spec.layers[:-1], spec.layers[1:])]
    bs = [rng.uniform(-1, 1, n).astype(np.float32) for n in spec.layers[1:]]
    dx, dw, db = torch.from_numpy(x).cuda(), [torch.from_numpy(w).cuda() for w in ws], [torch.from_numpy(b).cuda() for b in bs]
    for mode in (32, 0):
        rt.set_skinny_f32(mode)
        acts, before = [torch.full((8, n), float("nan"), device="cuda") for n in spec.layers[1:]], rt.skinny_f32_stats()[0]
        pkg.ShardedMlp(spec, rt=rt).forward(dx, dw, db, acts)
        torch.cuda.synchronize()
        assert rt.skinny_f32_stats()[0] == before + (3 if mode else 0)
        inp = x.astype(np.float64)
        for l, (w, b) in enumerate(zip(ws, bs)):
            got, w64 = acts[l].cpu().numpy(), w.astype(np.float64)
            err = np.abs(got - np.maximum(inp @ w64 + b, 0))
            assert (err <= (w.shape[0] + 3) * 2.0 ** -24 * (np.abs(inp) @ np.abs(w64) + np.abs(b))).all(), (mode, l, err.max())
            inp = got.astype(np.float64)


if __name__ == "__main__":
    r = pkg.get_runtime()
    mode = r.set_skinny_f32(0)
    r.set_skinny_f32(mode)
    res, kernel = Case(*(int(x) for x in sys.argv[1:6])).run(r)
    print(json.dumps(dict(from_env=mode, strict=r.get_strict(), kernel=kernel, stats=list(r.skinny_f32_stats()), bits=res.view(np.uint32).tolist())))
