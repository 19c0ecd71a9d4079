"""bf16 ragged k (include/tpp_xsmm_abi.h xsmm_hip_set_edge_k_bf16) on a real MI355X: a whole-layer bf16 call whose k is a multiple of 16 but
not of 64 runs on brgemm_bf16_lw GRP = 4 - every batch element in ceil(k / 64) chunks, the last one shifted back to end at k, its re-read
16-k MFMA steps skipped.

Tiles t = 0 .. 3 (32x64 + K2, 64x64, 64x128, 128x128), B images VNNI-2 / flat / VNNI-4. For a tile (bm, bn) the shapes are (2 bm, 2 bn)
under the switch alone and (bm + 1, bn + 8) with edge-tile mode 20 + t forcing the same tile as well; k in {80, 96, 112, 160, 272, 560} -
3, 2, 1, 2, 3, 1 skipped steps and 2, 2, 2, 3, 5, 9 chunks per element: a K group of the K2 tile skipping its whole share, more chunks
than the 4-slot and than the 8-slot ring - with 1 and 3 batch elements.
  1 exact inputs (tests/exact_data.py), bit for bit against the oracle: every tile and image, four epilogues - the strided ones with a
    gap behind every batch element of an A row, rows behind every B element, padded ldb / ldc and moved base pointers, one of them with
    poison in all of that and around C; then the reported kernel and the four counters; the edge-tile and f32 ragged-k counters unmoved
  2 one +Inf in the re-read region of A or of B among positive operands: the oracle's result - +Inf in that row or column, no NaN
  3 random operands: within one bf16 ulp of the oracle; the same bits on a second run and, in a process of its own, in strict mode
  4 mode 1: the reported tile is the rule's (tests/test_gemm_plan_edge_k_bf16.py kedge_rule = tests/golden/gemm_plan_edge_k_bf16.txt)
  5 ineligible calls: the kernel and the bits of mode 0, the counters do not move
  6 host pointers   7 more tiles than the chip holds at once, beta = 1 + bias   8 the set functions
Every case resets all three modes to 0."""
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
from test_gemm_plan_edge_k_bf16 import kedge_rule
from test_parity_gpu import F32, check_close, gemm_case

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]  # mode 20 + t -> output tile
TILE_NAME = ["<32x64,k2>", "<64x64>", "<64x128>", "<128x128>"]
FAMILY = {2: "brgemm_bf16_lw", 0: "brgemm_bf16_lw_flatb", 4: "brgemm_bf16_lw_vnni4"}  # B image -> kernel family
BASE = {2: 20, 0: 24, 4: 28}                                                           # ... -> variant number of its 32x64 + K2 tile
KS = (80, 96, 112, 160, 272, 560)
assert [(64 - k % 64) // 16 for k in KS] == [3, 2, 1, 2, 3, 1] and [-(-k // 64) for k in KS] == [2, 2, 2, 3, 5, 9]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def all_modes_off(rt):
    rt.set_edge_k_bf16(0), rt.set_edge_k(0), rt.set_edge_tiles(0)
    yield
    rt.set_edge_k_bf16(0), rt.set_edge_k(0), rt.set_edge_tiles(0)


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def counters(rt):
    return rt.edge_k_bf16_stats(), rt.edge_tiles_stats(), rt.edge_k_stats()


def assert_ragged_k_launch(rt, before, t, image, k, edge):
    """the launch just made ran on the ragged-k instance of tile t with B image `image`: the reported kernel, the counters as computed
    from k; the edge-tile and the f32 ragged-k counters have not moved"""
    refined, after = rt.last_refined_kernel(), counters(rt)
    assert refined == FAMILY[image] + TILE_NAME[t] + (", edge tiles, ragged k" if edge else ", ragged k"), refined
    assert after[0] == (before[0][0] + 1, -(-k // 64), 64 - k % 64, BASE[image] + t), (before, after, k)
    assert after[1:] == before[1:]


EPILOGUES = {"beta0": dict(beta0=True), "beta1_bias_relu": dict(bias=True, relu=True),
             "strided": dict(beta0=True, bias=True, strided=True), "poison": dict(beta0=True, bias=True, relu=True, strided=True, poison=True)}


def exact_call(rt, t, image, m, n, k, br, ep, seed, edge, mode="device", ek=None):
    """gemm_case on exact inputs under edge_k_bf16 mode 20 + t (edge: edge-tile mode 20 + t forces the same tile as well): bit for bit the
    oracle's, nothing written outside the m x n window (with poison: and nothing read outside the operand windows); then the kernel and
    the counters"""
    kw = dict(EPILOGUES[ep] if isinstance(ep, str) else ep)
    if kw.pop("strided", False):  # a gap behind every batch element of a row, four k-rows behind every B element, ldb and ldc padded, every base pointer moved
        kw.update(lda=br * (k + 8) + 8, sa=k + 8, ldb=n + 8, ldc=n + 16, sb=(k + 4) * (n + 8), offs=(8, 16, 8, 4))
    else:
        kw.update(lda=k * br, sa=k, ldb=n, sb=k * n)
    rt.set_edge_k_bf16(20 + t if ek is None else ek), rt.set_edge_tiles(20 + t if edge is True else edge or 0)
    before = counters(rt)
    with b_image(rt, image):
        gemm_case(rt, BF16, m, n, k, br, vnni=bool(image), values="exact", ranges=ed.exact_ranges(BF16, k * br), seed=seed, mode=mode, **kw)
    assert_ragged_k_launch(rt, before, t, image, k, bool(edge))


@pytest.mark.parametrize("br", [1, 3])
@pytest.mark.parametrize("ep", sorted(EPILOGUES))
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_bit_for_bit_against_the_oracle(rt, t, image, ep, br):
    """Without the skip (bkedge_step_runs always true) this fails on every tile with wrong sums: DESIGN 4.6e has the counts"""
    bm, bn = TILE[t]
    for i, k in enumerate(KS):
        exact_call(rt, t, image, 2 * bm, 2 * bn, k, br, ep, 1000 * t + 100 * image + 10 * i + br, edge=False)
        exact_call(rt, t, image, bm + 1, bn + 8, k, br, ep, 5000 + 1000 * t + 100 * image + 10 * i + br, edge=True)


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("k", [80, 96, 160])
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_an_inf_in_the_overlap_counts_once(rt, t, image, k, where):
    """all operands positive integers, one +Inf at a k that the last chunk holds again: skipped, it gives +Inf in its row (A) or column
    (B) and nothing else; multiplied by a zero it would give NaN"""
    bm, bn = TILE[t]
    m, n, br, o = 2 * bm, 2 * bn, 3, 64 - k % 64
    rng = np.random.default_rng(1000 * t + 10 * k + image)
    ra, rb, rc = ed.exact_ranges(BF16, k * br)
    A, B, C, D = (orc.f32_to_bf16(rng.integers(1, max(r, 2), s + 8).astype(np.float32)) for s, r in ((m * k * br, ra), (k * br * n, rb), (m * n, rc), (n, rc)))
    kk = k - 64 + (o // 2)  # inside [k - 64, k - 64 + o): the re-read region of the last chunk
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
    rt.set_edge_k_bf16(20 + t)
    before = counters(rt)
    got, _ = layer_call(rt, image, m, n, k, br, A, B, C, D)
    assert_ragged_k_launch(rt, before, t, image, k, False)
    g, r = (orc.bf16_to_f32(x[:m * n]).reshape(m, n) for x in (got, ref))
    assert not np.isnan(g).any(), "%d NaN: the overlap was multiplied" % int(np.isnan(g).sum())
    want_inf = np.zeros((m, n), bool)
    if where == "A":
        want_inf[i, :] = True
    else:
        want_inf[:, j] = True
    assert np.array_equal(np.isposinf(r), want_inf) and np.array_equal(np.isposinf(g), want_inf)
    ed.check_bits(got[:m * n], ref[:m * n], BF16, "inf in %s, tile %d image %d k %d" % (where, t, image, k), special=True)


@pytest.mark.parametrize("k,br", [(80, 3), (160, 1), (560, 3)])
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_within_one_ulp_and_repeatable(rt, t, image, k, br):
    bm, bn = TILE[t]
    m, n = 2 * bm, 2 * bn
    A, B, C, D = operands(m, n, k, br, 31 * t + 7 * image + k)
    ref = C.copy()
    with b_image(rt, image):
        orc.fused_brgemm(BF16, m, n, k, k * br, n, n, k, k * n, VB if image else 0, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, br)
    rt.set_edge_k_bf16(20 + t)
    before = counters(rt)
    got, refined = layer_call(rt, image, m, n, k, br, A, B, C, D)
    assert_ragged_k_launch(rt, before, t, image, k, False)
    again, _ = layer_call(rt, image, m, n, k, br, A, B, C, D)
    assert np.array_equal(got, again), "a second run gave other bits"
    assert np.array_equal(got[m * n:], C[m * n:]), "wrote beyond the m x n window"
    check_close(got[:m * n], ref[:m * n], BF16, "bf16 ragged k %s m%d n%d k%d br%d" % (refined, m, n, k, br))


@pytest.mark.parametrize("t,image", [(0, 2), (1, 4), (3, 0)])
def test_strict_mode_same_kernel_same_bits(rt, t, image):
    bm, bn = TILE[t]
    m, n, k, br = 2 * bm, 2 * bn, 160, 3
    A, B, C, D = operands(m, n, k, br, 40 + t)
    rt.set_edge_k_bf16(20 + t)
    before = counters(rt)
    got, refined = layer_call(rt, image, m, n, k, br, A, B, C, D)
    assert_ragged_k_launch(rt, before, t, image, k, False)
    rt.set_edge_k_bf16(0)
    # strict mode is chosen before anything is queued: a fresh child process (the mode arrives through the environment there)
    drop = ("TPP_HIP_STRICT", "TPP_HIP_EDGE_K", "TPP_HIP_EDGE_K_BF16", "TPP_HIP_EDGE_TILES", "TPP_HIP_TAIL_SPLIT", "TPP_HIP_SPLIT", "TPP_HIP_VNNI_FACTOR")
    env = {k_: v for k_, v in os.environ.items() if k_ not in drop}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_EDGE_K_BF16=str(20 + t))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edge_k_bf16_worker.py")] + [str(x) for x in (20 + t, image, m, n, k, br, 40 + t)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["edge_k_bf16_from_env"] == 20 + t
    assert d["kernels"] == [refined] * 3, d["kernels"]
    assert d["stats"] == [3, 3, 32, BASE[image] + t]
    assert set(d["digests"]) == {digest(got)}, "strict mode takes the same decision: the same bits"


@pytest.mark.parametrize("m,n,k,et,image", [(1024, 1024, 784, 0, 2), (256, 1024, 400, 0, 2), (256, 1024, 400, 0, 0), (1000, 1000, 784, 2, 2)])
def test_mode_1_takes_the_tile_of_the_table(rt, m, n, k, et, image):
    """the rule with its gate: 256 x 1024 x 400 with a VNNI-2 B is planned on the 32x32 K-split kernel, whose 256 tiles fit one round of a
    256-CU chip, and stays there (measured slower on the tiles); with a flat B the same shape is the generic kernel's and is taken"""
    t = kedge_rule(m, n, k, 1, et, 1, cu_count())
    if cu_count() == 256:  # tests/golden/gemm_plan_edge_k_bf16.txt, the br1 cus256 rows
        assert t == {(1024, 1024): 1, (256, 1024): 0, (1000, 1000): 1}[(m, n)]
    if image == 2 and m % 32 == 0 and n % 32 == 0 and (m // 32) * (n // 32) <= cu_count() and k < 1024:  # the gate (a VNNI-2 B on 32x32 tiles: the K-split kernel)
        rt.set_edge_k_bf16(1)
        before = counters(rt)
        gemm_case(rt, BF16, m, n, k, 1, lda=k, sa=k, ldb=n, sb=k * n, bias=True, relu=True, vnni=True, values="exact", ranges=ed.exact_ranges(BF16, k), seed=m + n)
        assert "ragged k" not in rt.last_refined_kernel() and counters(rt) == before
        return
    exact_call(rt, t, image, m, n, k, 1, "beta1_bias_relu", m + n, edge=et, ek=1)


def test_the_set_function_refuses_other_values(rt):
    assert rt.set_edge_k_bf16(21) == 0 and rt.set_edge_k_bf16(1) == 21 and rt.set_edge_k_bf16(23) == 1
    for bad in (-1, 2, 6, 24):
        assert rt.set_edge_k_bf16(bad) == -1
    assert rt.set_edge_k_bf16(0) == 23
    # the two older switches refuse what they refused
    for bad in (-1, 2, 5, 8, 11, 20):
        assert rt.set_edge_k(bad) == -1
    for bad in (-1, 3, 5, 8, 11, 19, 24, 28, 31):
        assert rt.set_edge_tiles(bad) == -1
    assert rt.set_edge_k(0) == 0 and rt.set_edge_tiles(0) == 0


# (what, call): everything else about the call is eligible - m = 128, n = 256, k = 208, one batch element, a VNNI-2 B, 16-byte aligned
INELIGIBLE = [
    ("k = 72: not in 16-k steps", dict(k=72)),
    ("k = 1000: not in 16-k steps", dict(k=1000)),
    ("k = 48: below a chunk", dict(k=48)),
    ("k = 128: whole chunks", dict(k=128)),
    ("f32", dict(dt=F32)),
    ("the generic kernel forced", dict(force=8)),
    ("n = 260: no 16-byte pieces", dict(n=260)),
    ("m and n ragged with the edge tiles off", dict(m=129, n=264)),
]


@pytest.mark.parametrize("what,call", INELIGIBLE, ids=[c[0].split(":")[0] for c in INELIGIBLE])
def test_ineligible_calls_are_untouched(rt, what, call):
    kw = dict(m=128, n=256, k=208)
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
        rt.set_edge_k_bf16(mode)
        got, refined = call_()
        assert refined == want_refined and "ragged k" not in refined, (what, mode, refined, want_refined)
        assert np.array_equal(ed.bits(got), ed.bits(want)), (what, mode)
    assert counters(rt) == before, what


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_host_pointers(rt, t, image):
    bm, bn = TILE[t]
    exact_call(rt, t, image, 2 * bm, 2 * bn, 160, 3, "beta1_bias_relu", t, edge=False, mode="host")
    exact_call(rt, t, image, bm + 1, bn + 8, 96, 1, "beta1_bias_relu", t, edge=True, mode="host")


def test_more_tiles_than_can_be_resident_beta_1(rt):
    """64x64 at 1025 x 1096 x 80: 17 x 18 = 306 tiles, more than the chip holds at once (one workgroup per CU), ragged in all three
    dimensions. Tiles of a later round start after neighbours of an earlier one have stored: each of the three runs must be the oracle's bits"""
    m, n, k = 1025, 1096, 80
    assert -(-m // 64) * -(-n // 64) > cu_count()
    for _ in range(3):
        exact_call(rt, 1, 2, m, n, k, 1, dict(bias=True), 7, edge=True)
