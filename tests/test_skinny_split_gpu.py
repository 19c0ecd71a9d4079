"""The K split across workgroups of the skinny-batch bf16 kernel (include/tpp_xsmm_abi.h xsmm_hip_set_skinny_split) on a real MI355X: with
xsmm_hip_set_skinny_bf16 AND this switch on, a whole-layer bf16 call with 1 <= m <= 31 runs on ceil(n / BN) * P_eff workgroups of
brgemm_bf16_skinny_split<IMG, BN, MB> - the 32-k steps of a column block over P_eff = min(P, steps) workgroups, f32 partials parked in the
stream's scratch block, the last workgroup to arrive sums them in part order and runs the epilogue.

Every case runs under a forced BN (16, 32, 64) and a forced P (2 .. 16) and leaves both switches 0. (P, k, br) in {(2, 32, 2) one step a
part, (2, 72, 1) and (3, 72, 1) a ragged tail in the last part, (16, 72, 1) P_eff = 3 < P, (3, 64, 3) parts that are whole batch elements,
(3, 64, 16) parts of 11 / 11 / 10 steps - eight waves, runs that cross batch elements -, (16, 64, 16) sixteen parts of two waves, (2, 1000,
1), (16, 1000, 1)}; m in {1, 16, 17, 31}; n in {BN, BN + 8, 200}; B VNNI-2, flat and VNNI-4 on every BN that has an instance. Operands are
strided (tests/skinny_bf16_worker.py Case): every base pointer moved, guard rows / gap columns of NaN around the inputs, a bit pattern
around C, checked after every run.
  1 exact inputs, bit for bit the oracle's, beta 0 + bias + relu and beta 1 plain - after the case's own precondition: the oracle equals
    the fp64 result rounded once; nothing outside the m x n window is written
  2 an Inf counts once: k = 72 under P = 2 and 3, one +Inf at k = 67, in A or in B
  3 random operands against the oracle within the project's bf16 bar (check_close); three runs on NaN-refilled outputs, all finite,
    identical bits (a counter that was not reset, or a stale partial, shows here); the m x n window has the bits of the same elements
    of a LARGER problem under the same BN and P (m' = 16 or 31, n' = n + 2 BN + 8). No tolerance.
  4 a sequence on one stream - P = 16, 2, 3, unsplit, 16 on different n -: every run has the bits it has alone
  5 every taken call asserts the reported kernel, xsmm_hip_skinny_split_stats, xsmm_hip_skinny_bf16_stats and that the counters of the six
    other single-call switches stand still
  6 calls that stay: one step (k = 32 and k = 8) under P = 16 runs the unsplit skinny kernel; m = 32, an f32 call, a tile-queue group of two
    and every call with the skinny switch off stay where they are: the bits and the text of split mode 0, the split counter still
  7 TPP_HIP_SKINNY_BF16=32 TPP_HIP_SKINNY_SPLIT=3 TPP_HIP_STRICT=1 in a child process: the same kernel, the same bits (n = 200: in strict
    mode a call with m, n <= 64 runs as a tile-queue group of one, which never sees either switch)
  8 ShardedMlp(MlpSpec(batch=8, layers=[256, 200, 256, 64])) under skinny mode 1 and split mode 2: every layer a split launch"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from oracle import pyoracle as orc
from skinny_bf16_worker import BF16, Case, corner, digest, embedded, expected_stats, instance_exists
from skinny_bf16_worker import text as unsplit_text
from skinny_split_worker import expected_skinny_stats, expected_split_stats, parts, text
from test_parity_gpu import check_close

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = [1, 16, 17, 31]
PKBR = [(2, 32, 2), (2, 72, 1), (3, 72, 1), (16, 72, 1), (3, 64, 3), (3, 64, 16), (16, 64, 16), (2, 1000, 1), (16, 1000, 1)]
INSTANCES = [(image, bn) for image in (2, 0, 4) for bn in (16, 32, 64) if instance_exists(image, bn)]
EPS = (dict(beta0=True, bias=True, relu=True), dict(beta0=False, bias=False, relu=False))
VB = 2048
INF = 0x7F80


def widths(bn):
    return [bn, bn + 8, 200]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def modes_off(rt):
    rt.set_skinny_bf16(0)
    rt.set_skinny_split(0)
    yield
    rt.set_skinny_bf16(0)
    rt.set_skinny_split(0)


def other_counters(rt):
    return (rt.edge_tiles_stats(), rt.edge_k_stats(), rt.edge_k_bf16_stats(), rt.edge_k8_bf16_stats(), rt.dma256_images_stats(),
            rt.dma256_edge_stats())


def run_taken(rt, case, bn, P):
    """the call under BN `bn` and P parts: it ran split - the reported kernel, both counters, no other counter, nothing outside the window"""
    assert parts(P, case.k, case.br) >= 2
    rt.set_skinny_bf16(bn)
    rt.set_skinny_split(P)
    before, sbefore, others = rt.skinny_bf16_stats(), rt.skinny_split_stats(), other_counters(rt)
    got, refined, _ = case.run(rt)
    rt.set_skinny_split(0)
    rt.set_skinny_bf16(0)
    assert refined == text(case.image, case.m, bn), refined
    assert rt.skinny_split_stats() == expected_split_stats(sbefore[0] + 1, case.n, case.k, case.br, bn, P), (sbefore, rt.skinny_split_stats())
    assert rt.skinny_bf16_stats() == expected_skinny_stats(before[0] + 1, case.image, case.n, case.k, case.br, bn, P), (before, rt.skinny_bf16_stats())
    assert other_counters(rt) == others
    assert case.outside_untouched(got), "wrote outside the m x n window"
    return got


def run_stays(rt, case, bn, P, **kw):
    """the call under skinny mode `bn` and split mode P: the split counter still; returns the C buffer, the reported kernel, the
    descriptor's kernel and how far the skinny counter moved"""
    rt.set_skinny_bf16(bn)
    rt.set_skinny_split(P)
    before, sbefore = rt.skinny_bf16_stats(), rt.skinny_split_stats()
    got, refined, name = case.run(rt, **kw)
    rt.set_skinny_split(0)
    rt.set_skinny_bf16(0)
    assert "split" not in refined and rt.skinny_split_stats() == sbefore, (refined, sbefore, rt.skinny_split_stats())
    return got, refined, name, rt.skinny_bf16_stats()[0] - before[0]


@pytest.mark.parametrize("P,k,br", PKBR)
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_exact_inputs_bit_for_bit_against_the_oracle_and_windows_intact(rt, image, bn, P, k, br):
    for m in MS:
        for n in widths(bn):
            for i, ep in enumerate(EPS):
                case = Case(image, m, n, k, br, 1000 * image + 31 * m + n + 10 * k + br + i + P, exact=True, **ep)
                ref = case.oracle()
                assert np.array_equal(ref[case.win], case.fp64()), "not an exact case: the oracle is not the fp64 result rounded once"
                assert case.outside_untouched(ref)
                got = run_taken(rt, case, bn, P)
                ed.check_bits(got[case.win], ref[case.win], BF16, "%s P%d m%d n%d k%d br%d %s" % (text(image, m, bn), P, m, n, k, br, sorted(x for x in ep if ep[x])))


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_an_inf_counts_once(rt, image, bn, P, where):
    """k = 72: the last part's last step keeps one lane group (k = 64 .. 71). All operands positive integers, one +Inf there: +Inf in
    exactly its row (A) or column (B), no NaN - a partial summed twice, a zero on one side only, or a load beyond k, would show"""
    k = 72
    for m in (16, 31):
        n = bn + 8
        case = Case(image, m, n, k, 1, 5 * image + m + bn, exact=True, beta0=True, bias=True, relu=True)
        rng = np.random.default_rng(m + bn)
        ii, kk, jj = np.arange(m)[:, None], np.arange(k)[None, :], np.arange(n)[None, :]
        a_idx = (case.offs[0] + ii * case.lda + kk).reshape(-1)
        b_idx = case.b_index(0, np.arange(k)[:, None], jj).reshape(-1)
        case.A[a_idx] = orc.f32_to_bf16(rng.integers(1, 4, a_idx.size).astype(np.float32))
        case.B[b_idx] = orc.f32_to_bf16(rng.integers(1, 4, b_idx.size).astype(np.float32))
        r, c, kinf = m - 1, n - 3, 67
        if where == "A":
            case.A[case.offs[0] + r * case.lda + kinf] = INF
        else:
            case.B[case.b_index(0, np.array([[kinf]]), np.array([[c]])).reshape(-1)] = INF
        ref = case.oracle()
        got = run_taken(rt, case, bn, P)
        g = ed.as_f32(got[case.win]).reshape(m, n)
        want = np.zeros((m, n), bool)
        if where == "A":
            want[r, :] = True
        else:
            want[:, c] = True
        assert not np.isnan(g).any(), "a NaN: an Inf met a one-sided zero, or memory beyond k was read"
        assert np.array_equal(np.isposinf(g), want) and not np.isneginf(g).any()
        assert np.array_equal(got[case.win], ref[case.win])


@pytest.mark.parametrize("P,k,br", PKBR)
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_random_operands_against_the_oracle_and_against_a_larger_problem(rt, image, bn, P, k, br):
    i = 0
    for m in MS:
        bigm = 16 if m <= 16 else 31
        for n in widths(bn):
            ep = EPS[i % 2]  # the two epilogues alternate over (m, n); both meet every m and every n
            i += 1
            seed = 77 * image + 31 * m + n + 10 * k + br + P
            what = "%s P%d m%d n%d k%d br%d %s" % (text(image, m, bn), P, m, n, k, br, sorted(x for x in ep if ep[x]))
            # the corner of a larger problem under the same BN and P: more rows (another clamp), more column blocks (another shift, other
            # workgroup numbers for the same part)
            big = Case(image, bigm, n + 2 * bn + 8, k, br, seed, **ep)
            case = embedded(big, m, n, seed + 1)
            want = corner(big, run_taken(rt, big, bn, P), m, n)
            ref = case.oracle()
            first = None
            for step in range(3):
                got = run_taken(rt, case, bn, P)
                assert np.isfinite(ed.as_f32(got[case.win])).all(), "read poisoned memory or a stale partial: " + what
                if step == 0:
                    first = got
                    check_close(got[case.win], ref[case.win], BF16, what)
                    ed.check_bits(got[case.win], want, BF16, "against the corner of %d x %d: %s" % (big.m, big.n, what))
                else:
                    assert np.array_equal(got, first), "step %d differs: %s" % (step, what)


def test_a_sequence_on_one_stream_has_the_bits_of_each_run_alone(rt):
    """P = 16, 2, 3, unsplit, 16 on different n, queued on one stream without a wait between them: the launches share the stream's scratch
    block and its counters - each run has the bits it has when run alone"""
    bn, k, br = 32, 64, 16
    seq = [(16, 200), (2, 72), (3, 1000), (0, 136), (16, 40)]
    cases = [Case(2, 16, n, k, br, 40 + i) for i, (_, n) in enumerate(seq)]
    alone = []
    for (P, _), case in zip(seq, cases):
        if P:
            alone.append(run_taken(rt, case, bn, P))
        else:
            got, refined, _, moved = run_stays(rt, case, bn, 0)
            assert refined == unsplit_text(2, 16, bn) and moved == 1
            alone.append(got)
    handles = [c.dispatch(rt) for c in cases]
    bufs = [c.device() for c in cases]
    was_async = rt.set_async(True)
    sbefore = rt.skinny_split_stats()[0]
    try:
        rt.set_skinny_bf16(bn)
        for (P, _), case, h, (dA, dB, dC, dD) in zip(seq, cases, handles, bufs):
            rt.set_skinny_split(P)
            o = case.offs
            rt.fused_brgemm(BF16, h, dA, o[0], dB, o[1], dC, o[2], dD, o[3], br)
        rt.synchronize()
    finally:
        rt.set_skinny_split(0)
        rt.set_skinny_bf16(0)
        rt.set_async(was_async)
    assert rt.skinny_split_stats()[0] == sbefore + 4
    for i, (want, (_, _, dC, _)) in enumerate(zip(alone, bufs)):
        assert np.array_equal(dC.cpu().numpy().view(np.uint16), want), "run %d of the sequence (P, n) = %s differs from the run alone" % (i, seq[i])


@pytest.mark.parametrize("k", [32, 8])
def test_one_step_under_p_16_runs_the_unsplit_skinny_kernel(rt, k):
    for image, bn in INSTANCES:
        case = Case(image, 16, 200, k, 1, 9 + k)
        want, off_kernel, off_name, moved0 = run_stays(rt, case, bn, 0)
        got, refined, name, moved = run_stays(rt, case, bn, 16)
        assert off_kernel == unsplit_text(image, 16, bn) and (refined, name, moved) == (off_kernel, off_name, moved0) and moved == 1
        assert np.array_equal(got, want)


# (what, skinny mode, how the eligible call - VNNI-2, 16 x 200, k = 64, br = 2 - differs)
STAYS = [("m = 32", 64, dict(m=32)), ("the skinny switch off", 0, dict()), ("the skinny switch off, m = 1", 0, dict(m=1)),
         ("the skinny switch off, k = 1000", 0, dict(k=1000, br=1))]


@pytest.mark.parametrize("what,bn,kw", STAYS, ids=[s[0] for s in STAYS])
def test_calls_that_stay_under_p_3(rt, what, bn, kw):
    case = Case(2, kw.get("m", 16), 200, kw.get("k", 64), kw.get("br", 2), 5)
    want, off_kernel, off_name, moved0 = run_stays(rt, case, bn, 0)
    got, refined, name, moved = run_stays(rt, case, bn, 3)
    assert (refined, name, moved) == (off_kernel, off_name, moved0) and moved == 0 and "skinny" not in refined, (what, refined, off_kernel)
    assert np.array_equal(got, want), what


def test_the_eligible_call_of_the_stays_list_is_taken(rt):
    run_taken(rt, Case(2, 16, 200, 64, 2, 5), 64, 3)


def test_an_f32_call_stays_where_it_is(rt):
    from edge_tiles_worker import layer_call as f32_call, operands as f32_operands
    A, B, C, D = f32_operands(16, 64, 64, 5)
    seen = {}
    for P in (0, 16):
        rt.set_skinny_bf16(64)
        rt.set_skinny_split(P)
        before, sbefore = rt.skinny_bf16_stats(), rt.skinny_split_stats()
        got, refined = f32_call(rt, 16, 64, 64, A, B, C, D)
        rt.set_skinny_split(0)
        rt.set_skinny_bf16(0)
        assert rt.skinny_bf16_stats() == before and rt.skinny_split_stats() == sbefore
        seen[P] = (refined, digest(got.view(np.uint16)))
    assert seen[0] == seen[16], seen


def test_a_tile_queue_group_stays_where_it_is(rt):
    """two queued invokes of a 16 x 64 x 64 descriptor - a split launch as a single call - run as a tile-queue group: both counters
    still, the bits of split mode 0"""
    tile = Case(2, 16, 64, 64, 1, 8, beta0=True, strided=False, poison=False)
    ht = tile.dispatch(rt)
    results = {}
    for P in (0, 2):
        rt.set_skinny_bf16(64)
        rt.set_skinny_split(P)
        before, sbefore = rt.skinny_bf16_stats(), rt.skinny_split_stats()
        tA, tB, _, tD = tile.device()
        outs = [tile.device()[2] for _ in range(2)]
        was_async, was_q = rt.set_async(True), rt.set_tile_queue(1)
        try:
            groups = rt.tile_queue_stats()[0]
            for o in outs:
                rt.fused_brgemm(BF16, ht, tA, 0, tB, 0, o, 0, tD, 0, 1)
            rt.flush()
            rt.synchronize()
            assert rt.tile_queue_stats()[0] > groups, "the two tile invokes did not run as a group"
        finally:
            rt.set_tile_queue(was_q)
            rt.set_async(was_async)
            rt.set_skinny_split(0)
            rt.set_skinny_bf16(0)
        assert rt.skinny_bf16_stats() == before and rt.skinny_split_stats() == sbefore, (P, before, rt.skinny_bf16_stats())
        results[P] = [digest(o.cpu().numpy()) for o in outs]
    assert results[0] == results[2]
    run_taken(rt, tile, 64, 2)  # (and the same descriptor IS split as a single call)


def test_the_environment_form_in_a_strict_child_process(rt):
    image, m, n, k, br, seed, bn, P = 4, 17, 200, 72, 1, 21, 32, 3
    got = run_taken(rt, Case(image, m, n, k, br, seed), bn, P)
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("TPP_HIP_")}
    env.update(TPP_HIP_SKINNY_BF16=str(bn), TPP_HIP_SKINNY_SPLIT=str(P), TPP_HIP_STRICT="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "skinny_split_worker.py")] + [str(x) for x in (image, m, n, k, br, seed)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["from_env"] == [bn, P] and d["strict"] == 1 and d["kernels"] == [text(image, m, bn)] * 3, d
    assert tuple(d["split_stats"]) == expected_split_stats(3, n, k, br, bn, P)
    assert tuple(d["stats"]) == expected_skinny_stats(3, image, n, k, br, bn, P)
    assert set(d["digests"]) == {digest(got)}


def test_a_batch_8_mlp_through_sharded_mlp(rt):
    """MlpSpec(batch 8, layers 256 -> 200 -> 256 -> 64), bf16, bias + relu, call by call (8 rows: no chain): under skinny mode 1 and split
    mode 2 every layer is a split launch. Each layer within the bf16 bar of the oracle fed the GPU's own activations, identical bits over
    three steps"""
    import torch
    spec = pkg.MlpSpec(batch=8, layers=[256, 200, 256, 64])
    rng = np.random.default_rng(3)
    bf = lambda a: orc.f32_to_bf16(np.ascontiguousarray(a, dtype=np.float32).ravel())  # noqa: E731
    x = bf(rng.uniform(-1, 1, (8, 256)))
    ws = [rng.uniform(-0.5, 0.5, (k, n)).astype(np.float32) for k, n in zip(spec.layers[:-1], spec.layers[1:])]
    wv = [bf(w.reshape(w.shape[0] // 2, 2, w.shape[1]).transpose(0, 2, 1)) for w in ws]  # VNNI-2: [k / 2][n][2]
    bs = [bf(rng.uniform(-1, 1, n)) for n in spec.layers[1:]]
    dev = lambda a: torch.from_numpy(a.view(np.int16).copy()).cuda()  # noqa: E731
    dx, dw, db = dev(x), [dev(w) for w in wv], [dev(b) for b in bs]
    rt.set_skinny_bf16(1)
    rt.set_skinny_split(2)
    try:
        mlp = pkg.ShardedMlp(spec, rt=rt)
        steps = []
        for step in range(3):
            acts = [torch.full((8 * n,), 0x7FC0, dtype=torch.int16, device="cuda") for n in spec.layers[1:]]
            before, sbefore = rt.skinny_bf16_stats(), rt.skinny_split_stats()
            out = mlp.forward(dx, dw, db, acts)
            torch.cuda.synchronize()
            assert out is acts[-1] and mlp.last_step_fused is False
            assert rt.skinny_bf16_stats()[0] == before[0] + 3 and rt.skinny_split_stats()[0] == sbefore[0] + 3
            assert rt.skinny_split_stats()[1] == 2 and "skinny_split" in rt.last_refined_kernel()
            steps.append([a.cpu().numpy().view(np.uint16) for a in acts])
    finally:
        rt.set_skinny_split(0)
        rt.set_skinny_bf16(0)
    assert all(np.array_equal(a, b) for s in steps[1:] for a, b in zip(s, steps[0])), "the steps differ"
    inp = x
    for l, (k, n) in enumerate(zip(spec.layers[:-1], spec.layers[1:])):
        ref = np.zeros(8 * n, np.uint16)
        kk, br = (64, k // 64) if k % 64 == 0 else (k, 1)
        orc.fused_brgemm(BF16, 8, n, kk, k, n, n, kk, kk * n, VB | 4, 0, 5, 4, 1, inp, 0, wv[l], 0, ref, 0, bs[l], 0, br)
        check_close(steps[0][l], ref, BF16, "split MLP layer %d" % l)
        inp = steps[0][l]
