"""Skinny-batch bf16 layers (include/tpp_xsmm_abi.h xsmm_hip_set_skinny_bf16) on a real MI355X: with the switch on, a whole-layer bf16 call
with 1 <= m <= 31 runs on ceil(n / BN) workgroups of brgemm_bf16_skinny<IMG, BN, MB> - all m rows of one block of BN columns per workgroup,
B straight from global memory into the MFMA operand registers, the 32-k steps dealt over the waves of the workgroup.

All cases run under a forcing mode (16, 32, 64) and leave the switch 0. m in {1, 7, 16, 17, 31} (one and two accumulator sets, clamped
rows); n in {BN, BN + 8, 200} (one block, a shifted second block, several blocks with a shifted last one); (k, br) in {(32, 1) one step -
W - 1 waves idle -, (8, 1) one step with three lane groups masked, (72, 1) a ragged tail, (64, 3) strides that are not the packed ones,
(64, 16) more steps than waves, (1000, 1)}; B VNNI-2, flat and VNNI-4; BN 16, 32, 64 (flat: 32, 64). Operands are strided
(tests/dma256_images_worker.py Case): lda > k, ldb > n, ldc > n, every base pointer moved, guard rows / gap columns of NaN around the
inputs, a bit pattern around C, checked after every run.
  1 exact inputs, bit for bit the oracle's, beta 0 + bias + relu and beta 1 plain - after the case's own precondition: the oracle equals
    the fp64 result rounded once
  2 an Inf counts once: positive integer operands and one +Inf in the last step of k = 72, in a kept lane group, in A or in B
  3 random operands against the oracle within the project's bf16 bar (check_close), three steps on NaN-refilled outputs: all finite,
    identical bits
  4 random operands: the m x n window has the bits of the same elements of a LARGER problem on the same BN that holds the call in its
    corner (m' = 31, or 16 for m <= 16; n' = n + 2 BN + 8; the same k and br). No tolerance.
  5 every taken call asserts the reported kernel, the stats and that the counters of the six other single-call switches stand still
  6 calls that stay under mode 64: the bits, the kernel name and the stats of mode 0
  7 TPP_HIP_SKINNY_BF16=32 with TPP_HIP_STRICT=1 in a child process: the same kernel, the same bits (n = 200: in strict mode a call with
    m, n <= 64 runs as a tile-queue group of one, which never sees the switch)
  8 ShardedMlp(MlpSpec(batch=8, layers=[256, 200, 256, 64])) under mode 1 and mode 0"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from oracle import pyoracle as orc
from skinny_bf16_worker import BF16, KIND, Case, corner, digest, embedded, expected_stats, instance_exists, text
from test_parity_gpu import check_close

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = [1, 7, 16, 17, 31]
KBR = [(32, 1), (8, 1), (72, 1), (64, 3), (64, 16), (1000, 1)]
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
def mode_off(rt):
    rt.set_skinny_bf16(0)
    yield
    rt.set_skinny_bf16(0)


def other_counters(rt):
    return (rt.edge_tiles_stats(), rt.edge_k_stats(), rt.edge_k_bf16_stats(), rt.edge_k8_bf16_stats(), rt.dma256_images_stats(),
            rt.dma256_edge_stats())


def run_taken(rt, case, bn):
    """the call under mode `bn`: it ran on the skinny kernel with its image - the reported kernel, the stats, no other counter"""
    rt.set_skinny_bf16(bn)
    before, others = rt.skinny_bf16_stats(), other_counters(rt)
    got, refined, _ = case.run(rt)
    rt.set_skinny_bf16(0)
    assert refined == text(case.image, case.m, bn), refined
    assert rt.skinny_bf16_stats() == expected_stats(before[0] + 1, case.image, case.n, case.k, case.br, bn), (before, rt.skinny_bf16_stats())
    assert other_counters(rt) == others
    assert case.outside_untouched(got), "wrote outside the m x n window"
    return got


def run_stays(rt, case, mode, **kw):
    rt.set_skinny_bf16(mode)
    before = rt.skinny_bf16_stats()
    got, refined, name = case.run(rt, **kw)
    rt.set_skinny_bf16(0)
    assert "skinny" not in refined and rt.skinny_bf16_stats() == before, (refined, before, rt.skinny_bf16_stats())
    return got, refined, name


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_exact_inputs_bit_for_bit_against_the_oracle_and_windows_intact(rt, image, bn, k, br):
    for m in MS:
        for n in widths(bn):
            for i, ep in enumerate(EPS):
                case = Case(image, m, n, k, br, 1000 * image + 31 * m + n + 10 * k + br + i, exact=True, **ep)
                ref = case.oracle()
                assert np.array_equal(ref[case.win], case.fp64()), "not an exact case: the oracle is not the fp64 result rounded once"
                assert case.outside_untouched(ref)
                got = run_taken(rt, case, bn)
                ed.check_bits(got[case.win], ref[case.win], BF16, "%s m%d n%d k%d br%d %s" % (text(image, m, bn), m, n, k, br, sorted(x for x in ep if ep[x])))


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_an_inf_counts_once(rt, image, bn, where):
    """k = 72: the last step keeps one lane group (k = 64 .. 71). All operands positive integers, one +Inf there: +Inf in exactly its row
    (A) or column (B), no NaN - a zero on one side only, or a load beyond k (NaN in the gaps), would give one"""
    k = 72
    for m in (7, 31):
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
        got = run_taken(rt, case, bn)
        g = ed.as_f32(got[case.win]).reshape(m, n)
        want = np.zeros((m, n), bool)
        if where == "A":
            want[r, :] = True
        else:
            want[:, c] = True
        assert not np.isnan(g).any(), "a NaN: an Inf met a one-sided zero, or memory beyond k was read"
        assert np.array_equal(np.isposinf(g), want) and not np.isneginf(g).any()
        assert np.array_equal(got[case.win], ref[case.win])


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_random_operands_against_the_oracle_and_against_a_larger_problem(rt, image, bn, k, br):
    for m in MS:
        bigm = 16 if m <= 16 else 31
        for n in widths(bn):
            for i, ep in enumerate(EPS):
                seed = 77 * image + 31 * m + n + 10 * k + br + i
                what = "%s m%d n%d k%d br%d %s" % (text(image, m, bn), m, n, k, br, sorted(x for x in ep if ep[x]))
                # the corner of a larger problem on the same BN: more rows (another clamp), more column blocks (another shift)
                big = Case(image, bigm, n + 2 * bn + 8, k, br, seed, **ep)
                case = embedded(big, m, n, seed + 1)
                want = corner(big, run_taken(rt, big, bn), m, n)
                ref = case.oracle()
                first = None
                for step in range(3):
                    got = run_taken(rt, case, bn)
                    assert np.isfinite(ed.as_f32(got[case.win])).all(), "read poisoned memory: " + what
                    if step == 0:
                        first = got
                        check_close(got[case.win], ref[case.win], BF16, what)
                        ed.check_bits(got[case.win], want, BF16, "against the corner of %d x %d: %s" % (big.m, big.n, what))
                    else:
                        assert np.array_equal(got, first), "step %d differs: %s" % (step, what)


def test_an_f32_call_stays_where_it_is(rt):
    from edge_tiles_worker import layer_call as f32_call, operands as f32_operands
    A, B, C, D = f32_operands(16, 64, 64, 5)
    seen = {}
    for mode in (0, 64):
        rt.set_skinny_bf16(mode)
        before = rt.skinny_bf16_stats()
        got, refined = f32_call(rt, 16, 64, 64, A, B, C, D)
        rt.set_skinny_bf16(0)
        assert rt.skinny_bf16_stats() == before
        seen[mode] = (refined, digest(got.view(np.uint16)))
    assert seen[0] == seen[64], seen


# (what, how the eligible call - VNNI-2, 16 x 200, k = 64, br = 2 - differs)
STAYS = [("m = 32", dict(m=32)), ("a VNNI C", dict(vnni_c=True)), ("a forced generic kernel", dict(force=8)), ("n = 8", dict(n=8))]


@pytest.mark.parametrize("what,kw", STAYS, ids=[s[0] for s in STAYS])
def test_calls_that_stay_under_mode_64(rt, what, kw):
    kw = dict(kw)
    force, vnni_c = kw.pop("force", None), kw.pop("vnni_c", False)
    case = Case(2, kw.pop("m", 16), kw.pop("n", 200), 64, 2, 5)
    if vnni_c:
        base = case.flags()
        case.flags = lambda: base | 8192
    want, off_kernel, off_name = run_stays(rt, case, 0, force=force)
    got, refined, name = run_stays(rt, case, 64, force=force)
    assert (refined, name) == (off_kernel, off_name), (what, refined, off_kernel)
    assert np.array_equal(got, want), what


def test_the_eligible_call_of_the_stays_list_is_taken(rt):
    run_taken(rt, Case(2, 16, 200, 64, 2, 5), 64)


def test_a_tile_queue_group_stays_where_it_is(rt):
    """two queued invokes of a 16 x 64 x 64 descriptor - eligible as a single call - run as a tile-queue group: the counter still, the
    bits of mode 0"""
    tile = Case(2, 16, 64, 64, 1, 8, beta0=True, strided=False, poison=False)
    ht = tile.dispatch(rt)
    results = {}
    for mode in (0, 64):
        rt.set_skinny_bf16(mode)
        before = rt.skinny_bf16_stats()
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
        assert rt.skinny_bf16_stats() == before, (mode, before, rt.skinny_bf16_stats())
        results[mode] = [digest(o.cpu().numpy()) for o in outs]
    rt.set_skinny_bf16(0)
    assert results[0] == results[64]
    run_taken(rt, tile, 64)  # (and the same descriptor IS taken as a single call)


def test_the_environment_form_in_a_strict_child_process(rt):
    image, m, n, k, br, seed, bn = 4, 17, 200, 72, 1, 21, 32
    got = run_taken(rt, Case(image, m, n, k, br, seed), bn)
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("TPP_HIP_")}
    env.update(TPP_HIP_SKINNY_BF16=str(bn), TPP_HIP_STRICT="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "skinny_bf16_worker.py")] + [str(x) for x in (image, m, n, k, br, seed)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["from_env"] == bn and d["strict"] == 1 and d["kernels"] == [text(image, m, bn)] * 3, d
    assert tuple(d["stats"]) == expected_stats(3, image, n, k, br, bn)
    assert set(d["digests"]) == {digest(got)}


def test_a_batch_8_mlp_through_sharded_mlp(rt):
    """MlpSpec(batch 8, layers 256 -> 200 -> 256 -> 64), bf16, bias + relu: the chain is refused (8 rows) and runs call by call; under mode
    1 every call is the skinny kernel's, under mode 0 the generic kernel's. Each layer within the bf16 bar of the oracle fed the GPU's
    own activations, identical bits over three steps"""
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
    for mode in (1, 0):
        rt.set_skinny_bf16(mode)
        mlp = pkg.ShardedMlp(spec, rt=rt)
        steps = []
        for step in range(3):
            acts = [torch.full((8 * n,), 0x7FC0, dtype=torch.int16, device="cuda") for n in spec.layers[1:]]
            before = rt.skinny_bf16_stats()
            out = mlp.forward(dx, dw, db, acts)
            torch.cuda.synchronize()
            assert out is acts[-1] and mlp.last_step_fused is False
            assert rt.skinny_bf16_stats()[0] == before[0] + (3 if mode else 0)
            steps.append([a.cpu().numpy().view(np.uint16) for a in acts])
        rt.set_skinny_bf16(0)
        assert all(np.array_equal(a, b) for s in steps[1:] for a, b in zip(s, steps[0])), "mode %d: the steps differ" % mode
        inp = x
        for l, (k, n) in enumerate(zip(spec.layers[:-1], spec.layers[1:])):
            ref = np.zeros(8 * n, np.uint16)
            kk, br = (64, k // 64) if k % 64 == 0 else (k, 1)
            orc.fused_brgemm(BF16, 8, n, kk, k, n, n, kk, kk * n, VB | 4, 0, 5, 4, 1, inp, 0, wv[l], 0, ref, 0, bs[l], 0, br)
            check_close(steps[0][l], ref, BF16, "mode %d MLP layer %d" % (mode, l))
            inp = steps[0][l]
