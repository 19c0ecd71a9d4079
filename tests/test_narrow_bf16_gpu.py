"""Narrow-output bf16 layers (xsmm_hip_set_narrow_bf16) on a real MI355X, under the forcing modes: m in {32, 33, 47, 65, 200} (one block;
clamped rows in a single block and in a last block; several blocks), n in {1, 10, 16, 17, 31} (one accumulator set partly used, full, two
sets), (k, br) from one step with idle waves over masked lane groups and a ragged tail to more steps than waves, all three B images, every
BM. Operands are strided - lda > k, ldb > n, ldc = n + 3 (rows only 2-byte aligned), unpacked batch strides, every base pointer moved, C and
the bias by an odd element count -, NaN in every guard row and gap column, a bit pattern around C; every taken call asserts kernel and stats."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_data as ed  # noqa: E402
from dma256_images_worker import BF16, Case  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402
from test_parity_gpu import check_close  # noqa: E402

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
MS, NS = [32, 33, 47, 65, 200], [1, 10, 16, 17, 31]
KBR = [(32, 1), (8, 1), (72, 1), (64, 3), (64, 16), (1000, 1)]
INSTANCES = [(image, bm) for image in (2, 0, 4) for bm in (16, 32, 64)]  # Case.image: 2 VNNI-2, 0 flat, 4 VNNI-4
EPS = (dict(beta0=True, bias=True, relu=True), dict(beta0=False, bias=False, relu=False))
KIND, SUFFIX = {2: 0, 0: 2, 4: 4}, {2: "", 0: "_flatb", 4: "_vnni4"}  # Case.image -> what the stats report, the kernel text
INF = 0x7F80


class NarrowCase(Case):
    """dma256_images_worker.Case with the layout this kernel is for: ldc = n + 3 and ldb = n + 5 (odd n and odd leading dimensions), C moved by
    9 and the bias by 5 elements, A by 16 and B by 32 bytes; lda, both batch strides, the poison and the bit pattern around C as there.
    positive: integers 1 .. 3 in A, B and the bias (the Inf test)."""

    def __init__(self, image, m, n, k, br, seed, exact=False, positive=False, beta0=False, bias=True, relu=True, a_off=8):
        self.image, self.m, self.n, self.k, self.br, self.v = image, m, n, k, br, image or 1
        self.beta0, self.bias, self.relu = beta0, bias, relu
        self.lda, self.sa, self.ldb, self.ldc, self.offs = br * (k + 8) + 8, k + 8, n + 5, n + 3, (a_off, 16, 9, 5)
        self.sb, o = (k + 4) * self.ldb, self.offs
        sizes = (o[0] + (br - 1) * self.sa + m * self.lda + 8, o[1] + (br - 1) * self.sb + (k + 2) * self.ldb + 8, o[2] + m * self.ldc + 8, o[3] + n + 8)
        rng = np.random.default_rng(seed)
        if positive:
            self.A, self.B, self.C, self.D = (orc.f32_to_bf16(rng.integers(1, 4, s).astype(np.float32)) for s in sizes)
        elif exact:
            ra, rb, rc = ed.exact_ranges(BF16, k * br)
            self.A, self.B, self.C, self.D = (ed.exact_fill(rng, s, BF16, r) for s, r in zip(sizes, (ra, rb, rc, rc)))
        else:
            self.A, self.B, self.C, self.D = (orc.f32_to_bf16(rng.uniform(-s_, s_, s).astype(np.float32)) for s, s_ in zip(sizes, (1, 0.5, 1, 1)))
        self.win = (o[2] + np.arange(m)[:, None] * self.ldc + np.arange(n)[None, :]).reshape(-1)
        la, lb, _, ld_ = ed.live_masks(sizes, m, n, k, br, self.lda, self.ldb, self.ldc, self.sa, self.sb, o, vnni=bool(image), v=self.v, beta0=beta0, bias=bias)
        for arr, lv in zip((self.A, self.B, self.D), (la, lb, ld_)):
            arr[~lv] = ed.BF16_NAN
        keep = self.C[self.win].copy()
        self.C[:] = (np.arange(sizes[2], dtype=np.uint32) * 40503 + 12345).astype(np.uint16)  # the bit pattern around C
        self.C[self.win] = ed.BF16_NAN if beta0 else keep


@functools.lru_cache(maxsize=None)  # built once, shared by the three BM, never changed; its own precondition asserted for every case
def exact_case(image, m, n, k, br, i):
    case = NarrowCase(image, m, n, k, br, 1000 * image + 31 * m + n + 10 * k + br + i, exact=True, **EPS[i])
    ref = case.oracle()
    assert np.array_equal(ref[case.win], case.fp64()), "not an exact case: the oracle is not the fp64 result rounded once"
    assert case.outside_untouched(ref)
    return case, ref


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def mode_off(rt):
    rt.set_narrow_bf16(0)
    yield
    rt.set_narrow_bf16(0)


def other_counters(rt):
    return tuple(getattr(rt, s + "_stats")() for s in ("skinny_bf16", "skinny_split", "skinny_f32", "skinny_f32_split", "tail_split", "edge_tiles", "edge_k",
                                                        "edge_k_bf16", "edge_k8_bf16", "dma256_images", "dma256_edge"))


def run_taken(rt, case, bm):
    """the call under mode `bm`: the reported kernel, the stats, no other single-call switch's counter, nothing outside the m x n window"""
    rt.set_narrow_bf16(bm)
    before, others = rt.narrow_bf16_stats(), other_counters(rt)
    got, refined, _ = case.run(rt)
    rt.set_narrow_bf16(0)
    assert refined == "brgemm_bf16_narrow%s<%dx%d>" % (SUFFIX[case.image], bm, 16 if case.n <= 16 else 32), refined
    want = (before[0] + 1, -(-case.m // bm), min(8, case.br * -(-case.k // 32)), bm, KIND[case.image])
    assert rt.narrow_bf16_stats() == want, (before, rt.narrow_bf16_stats(), want)
    assert other_counters(rt) == others
    assert case.outside_untouched(got), "wrote outside the m x n window"
    return got


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("image,bm", INSTANCES)
def test_exact_inputs_bit_for_bit_against_the_oracle_and_windows_intact(rt, image, bm, k, br):
    for m, n, i in ((m, n, i) for m in MS for n in NS for i in range(len(EPS))):
        case, ref = exact_case(image, m, n, k, br, i)
        ed.check_bits(run_taken(rt, case, bm)[case.win], ref[case.win], BF16, "image %d bm %d m%d n%d k%d br%d ep %d" % (image, bm, m, n, k, br, i))


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("image,bm", INSTANCES)
def test_an_inf_counts_once(rt, image, bm, where):
    """k = 72: the last step keeps one lane group (k = 64 .. 71). All operands positive integers, one +Inf there: +Inf in exactly its row
    (A) or column (B), no NaN - a zero on one side only, or a load beyond k (NaN in the gaps), would give one"""
    for m, n in ((33, 10), (65, 31)):
        case, want = NarrowCase(image, m, n, 72, 1, 5 * image + m + bm, positive=True, beta0=True), np.zeros((m, n), bool)
        if where == "A":
            case.A[case.offs[0] + (m - 1) * case.lda + 67], want[m - 1, :] = INF, True
        else:
            case.B[case.b_index(0, np.array([[67]]), np.array([[n - 3]])).reshape(-1)], want[:, n - 3] = INF, True
        g = ed.as_f32(run_taken(rt, case, bm)[case.win]).reshape(m, n)
        assert not np.isnan(g).any() and np.array_equal(np.isposinf(g), want) and not np.isneginf(g).any()


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("image,bm", INSTANCES)
def test_random_operands_against_the_oracle_three_runs_identical(rt, image, bm, k, br):
    for m, n, i in ((33, 10, 0), (200, 31, 1), (65, 16, 0)):
        case = NarrowCase(image, m, n, k, br, 7 * image + m + n + k + br, **EPS[i])
        ref, runs = case.oracle(), [run_taken(rt, case, bm) for _ in range(3)]
        check_close(runs[0][case.win], ref[case.win], BF16, "image %d bm %d m%d n%d k%d br%d" % (image, bm, m, n, k, br))  # (asserts all finite)
        assert all(np.array_equal(r, runs[0]) for r in runs[1:])


STAYS = [("n = 32", dict(n=32), {}), ("m = 31", dict(m=31), {}), ("a forced variant", {}, dict(force=8)), ("A off 16 bytes", dict(a_off=4), {}), ("k = 12", dict(k=12), {})]


@pytest.mark.parametrize("what,kw,run_kw", STAYS, ids=[s[0] for s in STAYS])
def test_calls_that_stay_under_mode_32(rt, what, kw, run_kw):
    case = NarrowCase(**{**dict(image=2, m=64, n=16, k=64, br=2, seed=5), **kw})
    outs = []
    for mode in (0, 32):
        rt.set_narrow_bf16(mode)
        before = rt.narrow_bf16_stats()
        got, refined, name = case.run(rt, **run_kw)
        assert "narrow" not in refined and rt.narrow_bf16_stats() == before, (what, refined)
        outs.append((got.tobytes(), refined, name))
    assert outs[0] == outs[1], what
    run_taken(rt, NarrowCase(2, 64, 16, 64, 2, 5), 32)  # (the eligible call these differ from IS taken)


def test_an_f32_call_and_a_vnni_c_stay_under_mode_32(rt):
    from test_skinny_f32_gpu import Case as F32Case
    from edge_tiles_bf16_worker import VB, VC
    outs = []
    for mode in (0, 32):
        rt.set_narrow_bf16(mode)
        before = rt.narrow_bf16_stats()
        f32 = F32Case(64, 16, 64, 2, 5).run(rt)
        A, B = (orc.f32_to_bf16(np.random.default_rng(9).uniform(-1, 1, s).astype(np.float32)) for s in (64 * 64, 64 * 16))  # a VNNI C, packed, beta 0
        import torch
        dA, dB, dC = (torch.from_numpy(x.view(np.int16).copy()).cuda() for x in (A, B, np.zeros(64 * 16, np.uint16)))
        h = rt.brgemm_dispatch(BF16, 64, 16, 64, 64, 16, 16, 64 * 64, 64 * 16, 4 | VB | VC)
        rt.brgemm(BF16, h, dA, 0, dB, 0, dC, 0, 1)
        outs.append((f32[0].tobytes(), f32[1], dC.cpu().numpy().tobytes(), rt.last_refined_kernel()))
        assert "narrow" not in f32[1] + outs[-1][3] and rt.narrow_bf16_stats() == before
    assert outs[0] == outs[1]
