"""bf16 ragged k in half steps (include/tpp_xsmm_abi.h xsmm_hip_set_edge_k8_bf16) on a real MI355X: a whole-layer bf16 call whose k is a
multiple of 8 but not of 16 runs on brgemm_bf16_lw GRP = 6 - every batch element in ceil(k / 64) chunks, the last one shifted back to end at
k, its re-read whole 16-k MFMA steps skipped and, in the one step the overlap ends in the middle of, both MFMA operands zeroed in the lanes
that hold the lower eight k-values.

Tiles t = 0 .. 3 (32x64 + K2, 64x64, 64x128, 128x128), B images VNNI-2 / flat / VNNI-4. For a tile (bm, bn) the shapes are (2 bm, 2 bn)
under the switch alone and (bm + 1, bn + 8) with edge-tile mode 20 + t forcing the same tile as well; k in {72, 88, 104, 120, 168, 200, 296,
568} - overlaps 56, 40, 24, 8, 24, 56, 24, 8 and 2, 2, 2, 2, 3, 4, 5, 9 chunks per element: all four odd overlaps, a K group of the K2
tile that keeps nothing (56, 40), half a step (24) or one and a half steps (8) of a last chunk, more chunks than the 4-slot and than the
8-slot ring - with 1 and 3 batch elements.
  1 exact inputs (tests/exact_data.py), bit for bit against the oracle: every tile and image, four epilogues - the strided ones with a
    gap behind every batch element of an A row, rows behind every B element, padded ldb / ldc and moved base pointers, one of them with
    poison in all of that and around C; then the reported kernel and the four counters; the other three switches' counters unmoved
  2 one +Inf among positive operands, in the fully skipped steps, in the skipped half of the half step or in its kept half, in A or
    in B: the oracle's result - +Inf in that row or column, no NaN
  3 random operands: within one bf16 ulp of the oracle; the same bits on a second run and, in a process of its own, in strict mode
  4 mode 1: the reported tile is the rule's (tests/test_gemm_plan_edge_k8_bf16.py kedge8_rule = tests/golden/gemm_plan_edge_k8_bf16.txt)
  5 ineligible calls: the kernel and the bits of mode 0, no counter moves   6 both ragged-k switches on: each takes its own lengths
  7 host pointers   8 more tiles than the chip holds at once, beta = 1 + bias   9 the set functions   10 an MLP through ShardedMlp
Every case resets all four modes to 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from edge_k_bf16_worker import BF16, VB, b_image, digest, layer_call, operands
from oracle import pyoracle as orc
from test_gemm_plan_edge_k8_bf16 import V_GENERIC, V_SMALL32, kedge8_rule
from test_parity_gpu import F32, check_close, gemm_case

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]  # mode 20 + t -> output tile
TILE_NAME = ["<32x64,k2>", "<64x64>", "<64x128>", "<128x128>"]
FAMILY = {2: "brgemm_bf16_lw", 0: "brgemm_bf16_lw_flatb", 4: "brgemm_bf16_lw_vnni4"}  # B image -> kernel family
BASE = {2: 20, 0: 24, 4: 28}                                                           # ... -> variant number of its 32x64 + K2 tile
KS = (72, 88, 104, 120, 168, 200, 296, 568)
assert [64 - k % 64 for k in KS] == [56, 40, 24, 8, 24, 56, 24, 8] and [-(-k // 64) for k in KS] == [2, 2, 2, 2, 3, 4, 5, 9]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def all_modes_off(rt):
    rt.set_edge_k8_bf16(0), rt.set_edge_k_bf16(0), rt.set_edge_k(0), rt.set_edge_tiles(0)
    yield
    rt.set_edge_k8_bf16(0), rt.set_edge_k_bf16(0), rt.set_edge_k(0), rt.set_edge_tiles(0)


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def counters(rt):
    return rt.edge_k8_bf16_stats(), rt.edge_k_bf16_stats(), rt.edge_tiles_stats(), rt.edge_k_stats()


def assert_half_step_launch(rt, before, t, image, k, edge):
    """the launch just made ran on the half-step instance of tile t with B image `image`: the reported kernel, the counters as computed
    from k; the counters of the other three switches have not moved"""
    refined, after = rt.last_refined_kernel(), counters(rt)
    assert refined == FAMILY[image] + TILE_NAME[t] + (", edge tiles, ragged k, half step" if edge else ", ragged k, half step"), refined
    assert after[0] == (before[0][0] + 1, -(-k // 64), 64 - k % 64, BASE[image] + t), (before, after, k)
    assert after[1:] == before[1:]


EPILOGUES = {"beta0": dict(beta0=True), "beta1_bias_relu": dict(bias=True, relu=True),
             "strided": dict(beta0=True, bias=True, strided=True), "poison": dict(beta0=True, bias=True, relu=True, strided=True, poison=True)}


def exact_call(rt, t, image, m, n, k, br, ep, seed, edge, mode="device", ek=None):
    """gemm_case on exact inputs under edge_k8_bf16 mode 20 + t (edge: edge-tile mode 20 + t forces the same tile as well): bit for bit
    the oracle's, nothing written outside the m x n window (with poison: and nothing read outside the operand windows); then the kernel
    and the counters"""
    kw = dict(EPILOGUES[ep] if isinstance(ep, str) else ep)
    if kw.pop("strided", False):  # a gap behind every batch element of a row, four k-rows behind every B element, ldb and ldc padded, every base pointer moved
        kw.update(lda=br * (k + 8) + 8, sa=k + 8, ldb=n + 8, ldc=n + 16, sb=(k + 4) * (n + 8), offs=(8, 16, 8, 4))
    else:
        kw.update(lda=k * br, sa=k, ldb=n, sb=k * n)
    ra, rb, rc = ed.exact_ranges(BF16, k * br)
    assert k * br * ra * rb + 2 * rc * (1 + 2.0 ** -8) < 2 ** 24, "every partial sum is an integer an f32 holds: any order of adding gives the same bits"
    rt.set_edge_k8_bf16(20 + t if ek is None else ek), rt.set_edge_tiles(20 + t if edge is True else edge or 0)
    before = counters(rt)
    with b_image(rt, image):
        gemm_case(rt, BF16, m, n, k, br, vnni=bool(image), values="exact", ranges=(ra, rb, rc), seed=seed, mode=mode, **kw)
    assert_half_step_launch(rt, before, t, image, k, bool(edge))


@pytest.mark.parametrize("br", [1, 3])
@pytest.mark.parametrize("ep", sorted(EPILOGUES))
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_bit_for_bit_against_the_oracle(rt, t, image, ep, br):
    """Without the half-step handling - the half step run whole, or not at all - the sums are wrong on every tile: eight k-values of
    every batch element are counted twice or never"""
    bm, bn = TILE[t]
    for i, k in enumerate(KS):
        exact_call(rt, t, image, 2 * bm, 2 * bn, k, br, ep, 1000 * t + 100 * image + 10 * i + br, edge=False)
        exact_call(rt, t, image, bm + 1, bn + 8, k, br, ep, 5000 + 1000 * t + 100 * image + 10 * i + br, edge=True)


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("place", ["skipped steps", "skipped half", "kept half"])
@pytest.mark.parametrize("k", [72, 104, 168])
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_an_inf_in_the_overlap_counts_once(rt, t, image, k, place, where):
    """all operands positive integers, one +Inf at a k-value of the last chunk: in the whole steps that are skipped, in the skipped
    (lower) half of the half step - where it meets a zeroed partner: zeroed on one side only it would give NaN - or in the kept (upper)
    half. Each time +Inf in its row (A) or column (B) and nothing else"""
    bm, bn = TILE[t]
    m, n, br, o = 2 * bm, 2 * bn, 3, 64 - k % 64
    assert o % 16 == 8 and o >= 24
    lo, hi = {"skipped steps": (k - 64, k - 64 + o - 8), "skipped half": (k - 64 + o - 8, k - 64 + o), "kept half": (k - 64 + o, k - 64 + o + 8)}[place]
    rng = np.random.default_rng(1000 * t + 10 * k + image)
    ra, rb, rc = ed.exact_ranges(BF16, k * br)
    A, B, C, D = (orc.f32_to_bf16(rng.integers(1, max(r, 2), s + 8).astype(np.float32)) for s, r in ((m * k * br, ra), (k * br * n, rb), (m * n, rc), (n, rc)))
    kk = int(rng.integers(lo, hi))
    assert k - 64 <= kk < k
    i, j, b = bm + 3, bn + 5, 1
    inf = orc.f32_to_bf16(np.array([np.inf], np.float32))[0]
    with b_image(rt, image):
        v = orc.lib().oracle_get_vnni_factor()
        if where == "A":
            A[i * k * br + b * k + kk] = inf
        else:
            B[b * k * n + ed.b_live_index(kk, j, n, bool(image), v)] = inf
        ref = C.copy()
        orc.fused_brgemm(BF16, m, n, k, k * br, n, n, k, k * n, VB if image else 0, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, br)
    rt.set_edge_k8_bf16(20 + t)
    before = counters(rt)
    got, _ = layer_call(rt, image, m, n, k, br, A, B, C, D)
    assert_half_step_launch(rt, before, t, image, k, False)
    g, r = (orc.bf16_to_f32(x[:m * n]).reshape(m, n) for x in (got, ref))
    assert not np.isnan(g).any(), "%d NaN: an Inf met a zero" % int(np.isnan(g).sum())
    want_inf = np.zeros((m, n), bool)
    if where == "A":
        want_inf[i, :] = True
    else:
        want_inf[:, j] = True
    assert np.array_equal(np.isposinf(r), want_inf) and np.array_equal(np.isposinf(g), want_inf)
    ed.check_bits(got[:m * n], ref[:m * n], BF16, "inf in %s (%s), tile %d image %d k %d" % (where, place, t, image, k), special=True)


@pytest.mark.parametrize("k,br", [(72, 3), (168, 1), (568, 3)])
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_within_one_ulp_and_repeatable(rt, t, image, k, br):
    bm, bn = TILE[t]
    m, n = 2 * bm, 2 * bn
    A, B, C, D = operands(m, n, k, br, 31 * t + 7 * image + k)
    ref = C.copy()
    with b_image(rt, image):
        orc.fused_brgemm(BF16, m, n, k, k * br, n, n, k, k * n, VB if image else 0, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, br)
    rt.set_edge_k8_bf16(20 + t)
    before = counters(rt)
    got, refined = layer_call(rt, image, m, n, k, br, A, B, C, D)
    assert_half_step_launch(rt, before, t, image, k, False)
    again, _ = layer_call(rt, image, m, n, k, br, A, B, C, D)
    assert np.array_equal(got, again), "a second run gave other bits"
    assert np.array_equal(got[m * n:], C[m * n:]), "wrote beyond the m x n window"
    check_close(got[:m * n], ref[:m * n], BF16, "bf16 half-step ragged k %s m%d n%d k%d br%d" % (refined, m, n, k, br))


@pytest.mark.parametrize("t,image", [(0, 2), (1, 4), (3, 0)])
def test_strict_mode_same_kernel_same_bits(rt, t, image):
    bm, bn = TILE[t]
    m, n, k, br = 2 * bm, 2 * bn, 168, 3
    A, B, C, D = operands(m, n, k, br, 40 + t)
    rt.set_edge_k8_bf16(20 + t)
    before = counters(rt)
    got, refined = layer_call(rt, image, m, n, k, br, A, B, C, D)
    assert_half_step_launch(rt, before, t, image, k, False)
    rt.set_edge_k8_bf16(0)
    # strict mode is chosen before anything is queued: a fresh child process (the mode arrives through the environment there)
    drop = ("TPP_HIP_STRICT", "TPP_HIP_EDGE_K", "TPP_HIP_EDGE_K_BF16", "TPP_HIP_EDGE_K8_BF16", "TPP_HIP_EDGE_TILES", "TPP_HIP_TAIL_SPLIT", "TPP_HIP_SPLIT",
            "TPP_HIP_VNNI_FACTOR")
    env = {k_: v for k_, v in os.environ.items() if k_ not in drop}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_EDGE_K8_BF16=str(20 + t))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edge_k8_bf16_worker.py")] + [str(x) for x in (20 + t, image, m, n, k, br, 40 + t)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["edge_k8_bf16_from_env"] == 20 + t
    assert d["kernels"] == [refined] * 3, d["kernels"]
    assert d["stats"] == [3, 3, 24, BASE[image] + t]
    assert [s[0] for s in d["older_stats"]] == [0, 0, 0]
    assert set(d["digests"]) == {digest(got)}, "strict mode takes the same decision: the same bits"


@pytest.mark.parametrize("m,n,k,et,image", [(1024, 1024, 1000, 0, 2), (256, 1024, 200, 0, 2), (256, 1024, 200, 0, 0), (1000, 1000, 1000, 2, 2)])
def test_mode_1_takes_the_tile_of_the_table(rt, m, n, k, et, image):
    """the rule with its gate, which asks where the call is planned with the switch off: on the 32x32 K-split kernel, 256 tiles in one
    round of the chip and k < 1024, it stays. That kernel takes a k in 16-k steps only, so a call of this switch is the generic kernel's
    with every image - 256 x 1024 x 200 too, with a VNNI-2 B as with a flat one (tests/golden/gemm_plan_edge_k8_bf16.txt) - and is taken"""
    A, B, C, D = operands(m, n, k, 1, m + n)
    rt.set_edge_tiles(et)
    want, off = layer_call(rt, image, m, n, k, 1, A, B, C, D)  # where the call is with the switch off
    assert "ragged k" not in off
    t = kedge8_rule(m, n, k, 1, et, 1, cu_count(), V_SMALL32 if "small32" in off else V_GENERIC)
    if cu_count() == 256:  # tests/golden/gemm_plan_edge_k8_bf16.txt, the br1 cus256 rows
        assert t == {(1024, 1024): 1, (256, 1024): 0, (1000, 1000): 1}[(m, n)]
    if t is None:  # gated: untouched
        rt.set_edge_k8_bf16(1)
        before = counters(rt)
        got, refined = layer_call(rt, image, m, n, k, 1, A, B, C, D)
        assert refined == off and counters(rt) == before and np.array_equal(got, want)
        return
    exact_call(rt, t, image, m, n, k, 1, "beta1_bias_relu", m + n, edge=et, ek=1)


def test_the_set_function_refuses_other_values(rt):
    assert rt.set_edge_k8_bf16(21) == 0 and rt.set_edge_k8_bf16(1) == 21 and rt.set_edge_k8_bf16(23) == 1
    assert rt.set_edge_k8_bf16(20) == 23 and rt.set_edge_k8_bf16(22) == 20 and rt.set_edge_k8_bf16(23) == 22
    for bad in (-1, 2, 6, 19, 24):
        assert rt.set_edge_k8_bf16(bad) == -1
    assert rt.set_edge_k8_bf16(0) == 23
    assert rt.set_edge_k_bf16(0) == 0, "a switch of its own"
    # the three older switches refuse what they refused
    for bad in (-1, 2, 6, 24):
        assert rt.set_edge_k_bf16(bad) == -1
    for bad in (-1, 2, 5, 8, 11, 20):
        assert rt.set_edge_k(bad) == -1
    for bad in (-1, 3, 5, 8, 11, 19, 24, 28, 31):
        assert rt.set_edge_tiles(bad) == -1
    assert rt.set_edge_k_bf16(0) == 0 and rt.set_edge_k(0) == 0 and rt.set_edge_tiles(0) == 0


# (what, call): everything else about the call is eligible - m = 128, n = 256, k = 200, one batch element, a VNNI-2 B, 16-byte aligned
INELIGIBLE = [
    ("k = 80: the older switch's", dict(k=80)),
    ("k = 76: not in 8-k half steps", dict(k=76)),
    ("k = 56: below a chunk", dict(k=56)),
    ("k = 128: whole chunks", dict(k=128)),
    ("f32", dict(dt=F32)),
    ("the generic kernel forced", dict(force=8)),
    ("n = 260: no 16-byte pieces", dict(n=260)),
    ("m and n ragged with the edge tiles off", dict(m=129, n=264)),
]


@pytest.mark.parametrize("what,call", INELIGIBLE, ids=[c[0].split(":")[0] for c in INELIGIBLE])
def test_ineligible_calls_are_untouched(rt, what, call):
    kw = dict(m=128, n=256, k=200)
    kw.update(call)
    m, n, k, dt = kw.pop("m"), kw.pop("n"), kw.pop("k"), kw.pop("dt", BF16)
    if dt == F32:
        from edge_k_worker import layer_call as f32_call, operands as f32_operands
        A, B, C, D = f32_operands(m, n, k, 1, 11)
        call_ = lambda: f32_call(rt, m, n, k, 1, A, B, C, D)  # noqa: E731
    else:
        A, B, C, D = operands(m, n, k, 1, 11)
        call_ = lambda: layer_call(rt, 2, m, n, k, 1, A, B, C, D, **kw)  # noqa: E731
    before = counters(rt)
    want, want_refined = call_()
    for mode in (1, 20, 21):
        rt.set_edge_k8_bf16(mode)
        got, refined = call_()
        assert refined == want_refined and "ragged k" not in refined, (what, mode, refined, want_refined)
        assert np.array_equal(ed.bits(got), ed.bits(want)), (what, mode)
    assert counters(rt) == before, what


def test_both_ragged_k_switches_on_each_takes_its_own_lengths(rt):
    m, n = 128, 128
    rt.set_edge_k8_bf16(21), rt.set_edge_k_bf16(21)
    before = counters(rt)
    A, B, C, D = operands(m, n, 1000, 1, 5)
    ref = C.copy()
    orc.fused_brgemm(BF16, m, n, 1000, 1000, n, n, 1000, 1000 * n, VB, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, 1)
    got, refined = layer_call(rt, 2, m, n, 1000, 1, A, B, C, D)
    mid = counters(rt)
    assert refined == "brgemm_bf16_lw<64x64>, ragged k, half step" and mid[0] == (before[0][0] + 1, 16, 24, 21) and mid[1:] == before[1:]
    check_close(got[:m * n], ref[:m * n], BF16, "k = 1000 with both switches on")
    A, B, C, D = operands(m, n, 784, 1, 6)
    ref = C.copy()
    orc.fused_brgemm(BF16, m, n, 784, 784, n, n, 784, 784 * n, VB, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, 1)
    got, refined = layer_call(rt, 2, m, n, 784, 1, A, B, C, D)
    after = counters(rt)
    assert refined == "brgemm_bf16_lw<64x64>, ragged k" and after[1] == (mid[1][0] + 1, 13, 48, 21)
    assert after[0] == mid[0] and after[2:] == mid[2:]
    check_close(got[:m * n], ref[:m * n], BF16, "k = 784 with both switches on")


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_host_pointers(rt, t, image):
    bm, bn = TILE[t]
    exact_call(rt, t, image, 2 * bm, 2 * bn, 168, 3, "beta1_bias_relu", t, edge=False, mode="host")
    exact_call(rt, t, image, bm + 1, bn + 8, 104, 1, "beta1_bias_relu", t, edge=True, mode="host")


def test_more_tiles_than_can_be_resident_beta_1(rt):
    """64x64 at 1025 x 1096 x 72: 17 x 18 = 306 tiles, more than the chip holds at once (one workgroup per CU), ragged in all three
    dimensions. Tiles of a later round start after neighbours of an earlier one have stored: each of the three runs must be the oracle's bits"""
    m, n, k = 1025, 1096, 72
    assert -(-m // 64) * -(-n // 64) > cu_count()
    for _ in range(3):
        exact_call(rt, 1, 2, m, n, k, 1, dict(bias=True), 7, edge=True)


def test_an_mlp_with_a_200_wide_input_through_sharded_mlp(rt):
    """MlpSpec(batch 256, layers 200 -> 256 -> 256), bf16, bias + relu, with the switch at 21: layer 0 is ONE batch element of k = 200 on
    the half-step 64x64 tile, layer 1 (k = 256) the plain kernels'; each layer within one bf16 ulp of the oracle fed the GPU's own
    activations"""
    import torch
    spec = pkg.MlpSpec(batch=256, layers=[200, 256, 256])
    rng = np.random.default_rng(3)
    bf = lambda a: orc.f32_to_bf16(np.ascontiguousarray(a, dtype=np.float32).ravel())  # noqa: E731
    x = bf(rng.uniform(-1, 1, (256, 200)))
    ws = [rng.uniform(-0.5, 0.5, (k, n)).astype(np.float32) for k, n in zip(spec.layers[:-1], spec.layers[1:])]
    wv = [bf(w.reshape(w.shape[0] // 2, 2, w.shape[1]).transpose(0, 2, 1)) for w in ws]  # VNNI-2: [k / 2][n][2]
    bs = [bf(rng.uniform(-1, 1, n)) for n in spec.layers[1:]]
    dev = lambda a: torch.from_numpy(a.view(np.int16).copy()).cuda()  # noqa: E731
    dx, dw, db = dev(x), [dev(w) for w in wv], [dev(b) for b in bs]
    acts = [torch.zeros(256 * n, dtype=torch.int16, device="cuda") for n in spec.layers[1:]]
    rt.set_edge_k8_bf16(21)
    before = counters(rt)
    mlp = pkg.ShardedMlp(spec, rt=rt, chain=False)
    kernels = []
    cur = dx
    for l, (h, br) in enumerate(mlp.handles):  # forward()'s calls, one by one, to read what each reported
        rt.fused_brgemm(BF16, h, cur, 0, dw[l], 0, acts[l], 0, db[l], 0, br)
        kernels.append(rt.last_refined_kernel())
        cur = acts[l]
    assert [br for _, br in mlp.handles] == [1, 4]
    assert kernels[0] == "brgemm_bf16_lw<64x64>, ragged k, half step" and "ragged k" not in kernels[1], kernels
    after = counters(rt)
    assert after[0] == (before[0][0] + 1, 4, 56, 21) and after[1:] == before[1:]
    for a in acts:
        a.zero_()
    out = mlp.forward(dx, dw, db, acts)  # the product's path gives the same bits
    torch.cuda.synchronize()
    assert out is acts[-1] and counters(rt)[0][0] == after[0][0] + 1
    inp = x
    for l, (k, n) in enumerate(zip(spec.layers[:-1], spec.layers[1:])):
        got = acts[l].cpu().numpy().view(np.uint16)
        ref = np.zeros(256 * n, np.uint16)
        orc.fused_brgemm(BF16, 256, n, k, k, n, n, k, k * n, VB | 4, 0, 5, 4, 1, inp, 0, wv[l], 0, ref, 0, bs[l], 0, 1)
        check_close(got, ref, BF16, "MLP layer %d (%s)" % (l, kernels[l]))
        inp = got
