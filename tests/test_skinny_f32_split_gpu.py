"""The K split across workgroups of the skinny-batch f32 kernel (xsmm_hip_set_skinny_f32_split) on a real MI355X, under forced BN x forced
P: the operands, poison and window checks are Case of tests/test_skinny_f32_gpu.py; every taken call asserts the reported kernel text and
both stats blocks."""
import numpy as np
import pytest

from test_skinny_f32_gpu import Case, EPS, F32, ed, rt  # noqa: F401  (rt: the module-scoped runtime fixture)

pytestmark = pytest.mark.gpu
# (P, k, br): one step per part | 3 steps, the masked one alone in the last part | 9 steps 3 / 2 / 2 / 2, masked steps first, last and inside
# a part | 32 steps 11 / 11 / 10 on 8 waves with uneven runs | 63 steps in 4- and 3-step parts, ragged k
PKBR = [(2, 32, 1), (2, 36, 1), (4, 36, 3), (3, 32, 16), (16, 1000, 1)]


@pytest.fixture(autouse=True)
def modes_off(rt):
    rt.set_skinny_f32(0), rt.set_skinny_f32_split(0)
    yield
    rt.set_skinny_f32(0), rt.set_skinny_f32_split(0)


def run_modes(rt, case, bn, split):
    """(the m x n window, kernel text, the moves of skinny_f32_split_stats[0] and skinny_f32_stats[0], both blocks after the call)"""
    rt.set_skinny_f32(bn), rt.set_skinny_f32_split(split)
    b_split, b_skinny = rt.skinny_f32_split_stats(), rt.skinny_f32_stats()
    got, text = case.run(rt)
    rt.set_skinny_f32(0), rt.set_skinny_f32_split(0)
    a_split, a_skinny = rt.skinny_f32_split_stats(), rt.skinny_f32_stats()
    return got, text, (a_split[0] - b_split[0], a_skinny[0] - b_skinny[0]), (a_split, a_skinny), (b_split, b_skinny)


def run_split(rt, case, bn, P):
    got, text, moved, (split, skinny), _ = run_modes(rt, case, bn, P)
    steps, blocks = case.br * -(-case.k // 16), -(-case.n // bn)
    p_eff = min(P, steps)
    assert text == "brgemm_f32_skinny_split<%dx%d>" % (16 if case.m <= 16 else 32, bn) and moved == (1, 1), (text, moved)
    assert split[1:] == (p_eff, blocks * p_eff) and skinny[1:] == (blocks * p_eff, min(8, -(-steps // p_eff)), bn), (split, skinny)
    return got


@pytest.mark.parametrize("P,k,br", PKBR)
@pytest.mark.parametrize("bn", [16, 32, 64])
def test_exact_bits_the_fp64_bound_three_runs_and_the_corner_of_a_larger_problem(rt, bn, P, k, br):
    for m, n, (i, ep) in ((m, n, e) for m in (1, 16, 17, 31) for n in (bn, bn + 4, 200) for e in enumerate(EPS)):
        what = "m%d n%d k%d br%d bn%d P%d beta0=%d" % (m, n, k, br, bn, P, ep["beta0"])
        # 1. integers in [-3, 3]: every partial is exact (9 br k < 2^24) - the fp64 result cast to f32, no tolerance: the unsplit kernel's bits
        case = Case(m, n, k, br, 31 * m + n + 10 * k + br + i, exact=True, **ep)
        ed.check_bits(run_split(rt, case, bn, P).reshape(-1), case.fp64()[0].astype(np.float32).reshape(-1), F32, "exact " + what)
        # 2. random: |got - ref64| <= (br k + 3) 2^-24 (sum |a b| + |c_in| + |bias|), the worst case of any summation order; three runs on
        # NaN-refilled outputs: finite, identical bits - whoever arrived last, and the counters were reset
        case = Case(m, n, k, br, 77 * m + n + 10 * k + br + i, **ep)
        runs, (ref, mag) = [run_split(rt, case, bn, P) for _ in range(3)], case.fp64()
        assert np.isfinite(runs[0]).all(), "read poisoned memory: " + what
        err, lim = np.abs(runs[0].astype(np.float64) - ref), (br * k + 3) * 2.0 ** -24 * mag
        print(what, "max err / bound %.3g" % (err / np.maximum(lim, 1e-300)).max())
        assert (err <= lim).all() and all(np.array_equal(r.view(np.uint32), runs[0].view(np.uint32)) for r in runs[1:]), what
        # 3. placement: the bits of the same elements of a larger problem (same k, br, BN, P) that holds the call in its corner
        big = run_split(rt, Case(16 if m <= 16 else 31, n + 2 * bn + 4, k, br, 1, corner_of=case, **ep), bn, P)
        ed.check_bits(runs[0].reshape(-1), big[:m, :n].reshape(-1), F32, "the corner of a larger problem: " + what)


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("bn", [16, 32, 64])
def test_an_inf_counts_once(rt, bn, where):
    """k = 36, P = 2: the masked last step (k = 32 .. 35, lane group 0 alone) is a part of its own. One +Inf at k = 33: +Inf in exactly its
    row (A) or column (B), no NaN - through the parked partial and the last arriver's sum"""
    for m in (7, 31):
        n = bn + 4
        case, want = Case(m, n, 36, 1, m + bn, exact=True, lo=1), np.zeros((m, n), bool)
        if where == "A":
            case.A[case.ia[0, m - 1, 33]], want[m - 1, :] = np.inf, True
        else:
            case.B[case.ib[0, 33, n - 3]], want[:, n - 3] = np.inf, True
        got = run_split(rt, case, bn, 2)
        assert not np.isnan(got).any() and np.array_equal(np.isposinf(got), want) and not np.isneginf(got).any()


def test_a_sequence_on_one_stream_has_the_bits_of_each_call_alone(rt):
    """13 blocks P 2, 2 blocks P 16, 13 blocks P 3 back to back in asynchronous mode, twice: they share the stream's counters and scratch"""
    import torch
    calls = [(Case(17, 204, 1000, 1, 1), 2), (Case(8, 32, 64, 4, 2), 16), (Case(31, 204, 36, 3, 3), 3)]
    alone = [run_split(rt, c, 16, P) for c, P in calls]
    hs = [rt.fused_brgemm_dispatch(*c.args(), 0, 5, 4, 1) for c, _ in calls]
    was = rt.set_async(True)
    try:
        for _ in range(2):
            dev = [[torch.from_numpy(x.copy()).cuda() for x in (c.A, c.B, c.C, c.D)] for c, _ in calls]
            torch.cuda.synchronize()
            rt.set_skinny_f32(16)
            for (c, P), h, (dA, dB, dC, dD) in zip(calls, hs, dev):
                rt.set_skinny_f32_split(P)
                rt.fused_brgemm(F32, h, dA, c.o[0], dB, c.o[1], dC, c.o[2], dD, c.o[3], c.br)
            rt.synchronize()
            rt.set_skinny_f32(0), rt.set_skinny_f32_split(0)
            for (c, _), d, want in zip(calls, dev, alone):
                assert np.array_equal(d[2].cpu().numpy()[c.ic].view(np.uint32), want.view(np.uint32))
    finally:
        rt.set_async(was)


@pytest.mark.parametrize("what,shape,P", [("one step under P 16", (8, 200, 16, 1), 16), ("4097 column blocks", (1, 65552, 32, 1), 2)])
def test_a_refused_split_runs_the_unsplit_skinny_kernel_of_the_same_bn(rt, what, shape, P):
    case = Case(*shape, 7, exact=True)
    got, text, moved, (_, skinny), _ = run_modes(rt, case, 16, P)
    assert text == "brgemm_f32_skinny<16x16>" and moved == (0, 1) and skinny[1:] == (-(-case.n // 16), min(8, -(-case.k // 16)), 16), (what, text, moved, skinny)
    ed.check_bits(got.reshape(-1), case.oracle().reshape(-1), F32, what)


def test_the_split_switch_alone_changes_nothing(rt):
    case = Case(16, 200, 64, 2, 5)
    off, on = run_modes(rt, case, 0, 0), run_modes(rt, case, 0, 3)
    assert on[1] == off[1] and "skinny" not in on[1] and on[2] == (0, 0) and on[3] == on[4] and np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
