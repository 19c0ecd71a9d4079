"""Ragged k (include/tpp_xsmm_abi.h xsmm_hip_set_edge_k) on a real MI355X: a whole-layer f32 call whose k is a multiple of 8 but not of
64 runs on brgemm_f32_lw_kedge - every batch element in ceil(k / 64) chunks, the last one shifted back to end at k, its re-read k-blocks
skipped by the MFMA waves.

For a tile (bm, bn) the shapes are (2 bm, 2 bn) under edge_k alone and (bm + 1, bn + 4) with the edge-tile mode forcing the same tile;
k in {72, 80, 96, 112, 120, 168, 280} - 7, 6, 4, 2, 1, 3, 5 skipped blocks: whole K groups skipped on the K2 and K4 tiles, three chunks, more
chunks than ring slots - with 1 and 3 batch elements.
  1 exact inputs (tests/exact_data.py), bit for bit against the oracle: every forced tile, four epilogues, one of them with poison between
    the rows of A (and behind k of every batch element of a row), behind row k - 1 of every B element and around C
  2 one +Inf in the overlap of A or of B among positive operands: the oracle's result - +Inf in that row or column, no NaN
  3 random operands: within the f32 bars against the oracle; the same bits on a second run and, in a process of its own, in strict mode
  4 mode 1: the reported tile is the rule's (tests/test_gemm_plan_edge_k.py = tests/golden/gemm_plan_edge_k.txt)
  5 ineligible calls: the kernel and the bits of mode 0, the counters do not move
  6 host pointers   7 a replayed tile-queue group of 64x64x96 items is untouched
Every case resets both modes to 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from edge_k_worker import BF16, digest, layer_call, operands
from oracle import pyoracle as orc
from test_gemm_plan_edge import edge_rule
from test_parity_gpu import F32, check_close, gemm_case

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = {6: (64, 64), 7: (64, 32), 9: (32, 32), 10: (128, 64)}  # mode = GemmVariant -> output tile
NAME = {6: "brgemm_f32_lw<64x64,k2>", 7: "brgemm_f32_lw<64x32,k4>", 9: "brgemm_f32_lw<32x32,k4>", 10: "brgemm_f32_lw<128x64,k1>"}
KS = (72, 80, 96, 112, 120, 168, 280)
assert [(64 - k % 64) // 8 for k in KS] == [7, 6, 4, 2, 1, 3, 5]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def both_modes_off(rt):
    rt.set_edge_k(0), rt.set_edge_tiles(0)
    yield
    rt.set_edge_k(0), rt.set_edge_tiles(0)


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_ragged_k_launch(rt, before, variant, k, edge):
    """the launch just made ran on brgemm_f32_lw_kedge on the tile of `variant`: the reported kernel, the counters as computed from k;
    the edge-tile counters have not moved"""
    refined, after = rt.last_refined_kernel(), rt.edge_k_stats()
    assert refined == NAME[variant] + (", edge tiles, ragged k" if edge else ", ragged k"), refined
    assert after == (before[0][0] + 1, -(-k // 64), 64 - k % 64, variant), (before, after, k)
    assert rt.edge_tiles_stats() == before[1]


EPILOGUES = {"beta0": dict(beta0=True), "beta1_bias_relu": dict(bias=True, relu=True),
             "strided": dict(beta0=True, bias=True, strided=True), "poison": dict(beta0=True, bias=True, relu=True, strided=True, poison=True)}


def exact_call(rt, variant, m, n, k, br, ep, seed, edge, mode="device"):
    """gemm_case on exact inputs under edge_k mode `variant` (edge: the edge-tile mode forces the same tile): bit for bit the oracle's,
    nothing written outside the m x n window (with poison: and nothing read outside the operand windows); then the kernel and the counters"""
    kw = dict(EPILOGUES[ep])
    if kw.pop("strided", False):  # lda > k br with a gap behind every batch element of a row, two rows behind every B element, ldb and ldc padded
        kw.update(lda=br * (k + 8) + 4, sa=k + 8, ldb=n + 4, ldc=n + 4, sb=(k + 2) * (n + 4), offs=(4, 8, 4, 4))
    else:
        kw.update(lda=k * br, sa=k, ldb=n, sb=k * n)
    rt.set_edge_k(variant), rt.set_edge_tiles(variant if edge else 0)
    before = (rt.edge_k_stats(), rt.edge_tiles_stats())
    gemm_case(rt, F32, m, n, k, br, values="exact", ranges=ed.exact_ranges(F32, k * br), seed=seed, mode=mode, **kw)
    assert_ragged_k_launch(rt, before, variant, k, edge)


@pytest.mark.parametrize("br", [1, 3])
@pytest.mark.parametrize("ep", sorted(EPILOGUES))
@pytest.mark.parametrize("variant", [6, 7, 9, 10])
def test_exact_inputs_bit_for_bit_against_the_oracle(rt, variant, ep, br):
    bm, bn = TILE[variant]
    for i, k in enumerate(KS):
        exact_call(rt, variant, 2 * bm, 2 * bn, k, br, ep, 1000 * variant + 10 * i + br, edge=False)
        exact_call(rt, variant, bm + 1, bn + 4, k, br, ep, 2000 * variant + 10 * i + br, edge=True)


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("k", [72, 96, 168])
@pytest.mark.parametrize("variant", [6, 7, 9, 10])
def test_an_inf_in_the_overlap_counts_once(rt, variant, k, where):
    """all operands positive integers, one +Inf at a k that the last chunk holds again: skipped, it gives +Inf in its row (A) or column
    (B) and nothing else; multiplied by a zero it would give NaN, added twice it would still be +Inf - the exact test catches that"""
    bm, bn = TILE[variant]
    m, n, br, o = 2 * bm, 2 * bn, 3, 64 - k % 64
    rng = np.random.default_rng(variant * k)
    ra, rb, rc = ed.exact_ranges(F32, k * br)
    A, B, C, D = (np.abs(ed.exact_fill(rng, s + 8, F32, r)) + 1 for s, r in ((m * k * br, ra - 1), (k * br * n, rb - 1), (m * n, rc - 1), (n, rc - 1)))
    kk = k - 64 + (o // 2)  # inside [k - 64, k - 64 + o): the re-read region of the last chunk
    i, j, b = bm + 3, bn + 5, 1
    if where == "A":
        A[i * k * br + b * k + kk] = np.inf
    else:
        B[(b * k + kk) * n + j] = np.inf
    ref = C.copy()
    orc.fused_brgemm(F32, m, n, k, k * br, n, n, k, k * n, 0, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, br)
    rt.set_edge_k(variant)
    before = (rt.edge_k_stats(), rt.edge_tiles_stats())
    got, _ = layer_call(rt, m, n, k, br, A, B, C, D)
    assert_ragged_k_launch(rt, before, variant, k, False)
    g, r = got[:m * n].reshape(m, n), ref[:m * n].reshape(m, n)
    assert not np.isnan(g).any(), "%d NaN: the overlap was multiplied" % int(np.isnan(g).sum())
    want_inf = np.zeros((m, n), bool)
    if where == "A":
        want_inf[i, :] = True
    else:
        want_inf[:, j] = True
    assert np.array_equal(np.isposinf(r), want_inf) and np.array_equal(np.isposinf(g), want_inf)
    ed.check_bits(got[:m * n], ref[:m * n], F32, "inf in %s, variant %d k %d" % (where, variant, k), special=True)


@pytest.mark.parametrize("k,br", [(72, 3), (168, 1), (280, 3)])
@pytest.mark.parametrize("variant", [6, 7, 9, 10])
def test_random_operands_within_the_f32_bars_and_repeatable(rt, variant, k, br):
    bm, bn = TILE[variant]
    m, n = 2 * bm, 2 * bn
    A, B, C, D = operands(m, n, k, br, 31 * variant + k)
    ref, mag = C.copy(), np.abs(C)
    orc.fused_brgemm(F32, m, n, k, k * br, n, n, k, k * n, 0, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, br)
    orc.fused_brgemm(F32, m, n, k, k * br, n, n, k, k * n, 0, 0, 0, 4, 1, np.abs(A), 0, np.abs(B), 0, mag, 0, np.abs(D), 0, br)
    rt.set_edge_k(variant)
    before = (rt.edge_k_stats(), rt.edge_tiles_stats())
    got, refined = layer_call(rt, m, n, k, br, A, B, C, D)
    assert_ragged_k_launch(rt, before, variant, k, False)
    again, _ = layer_call(rt, m, n, k, br, A, B, C, D)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "a second run gave other bits"
    assert np.array_equal(got[m * n:].view(np.uint32), C[m * n:].view(np.uint32)), "wrote beyond the m x n window"
    check_close(got[:m * n], ref[:m * n], F32, "ragged k %s m%d n%d k%d br%d" % (refined, m, n, k, br), mag[:m * n], k * br)


@pytest.mark.parametrize("variant", [6, 10])
def test_strict_mode_same_kernel_same_bits(rt, variant):
    bm, bn = TILE[variant]
    m, n, k, br = 2 * bm, 2 * bn, 168, 3
    A, B, C, D = operands(m, n, k, br, 40 + variant)
    rt.set_edge_k(variant)
    before = (rt.edge_k_stats(), rt.edge_tiles_stats())
    got, refined = layer_call(rt, m, n, k, br, A, B, C, D)
    assert_ragged_k_launch(rt, before, variant, k, False)
    rt.set_edge_k(0)
    # strict mode is chosen before anything is queued: a fresh child process (the mode arrives through the environment there)
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("TPP_HIP_STRICT", "TPP_HIP_EDGE_K", "TPP_HIP_EDGE_TILES", "TPP_HIP_TAIL_SPLIT", "TPP_HIP_SPLIT")}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_EDGE_K=str(variant))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edge_k_worker.py")] + [str(x) for x in (variant, m, n, k, br, 40 + variant)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["edge_k_from_env"] == variant
    assert d["kernels"] == [refined] * 3, d["kernels"]
    assert d["stats"] == [3, 3, 24, variant]
    assert set(d["digests"]) == {digest(got)}, "strict mode takes the same decision: the same bits"


@pytest.mark.parametrize("m,n,k,edge", [(1024, 1024, 72, 0), (512, 1024, 72, 0), (256, 1024, 200, 0), (1000, 1000, 72, 1), (1000, 1000, 72, 6)])
def test_mode_1_takes_the_tile_of_the_table(rt, m, n, k, edge):
    variant = edge if edge in TILE else edge_rule(m, n, 1, cu_count())
    if cu_count() == 256:  # tests/golden/gemm_plan_edge_k.txt, cus256 rows
        assert variant == {(1024, 1024): 6, (512, 1024): 7, (256, 1024): 9, (1000, 1000): 6}[(m, n)]
    rt.set_edge_k(1), rt.set_edge_tiles(edge)
    before = (rt.edge_k_stats(), rt.edge_tiles_stats())
    gemm_case(rt, F32, m, n, k, 1, bias=True, relu=True, values="exact", ranges=ed.exact_ranges(F32, k), seed=m + n)
    assert_ragged_k_launch(rt, before, variant, k, edge != 0)


def test_the_set_function_refuses_other_values(rt):
    assert rt.set_edge_k(6) == 0 and rt.set_edge_k(1) == 6
    for bad in (-1, 2, 5, 8, 11, 20):
        assert rt.set_edge_k(bad) == -1
    assert rt.set_edge_k(0) == 1


# (what, call): everything else about the call is eligible - m = 128, n = 256, k = 200, one batch element, row-major, 16-byte aligned
INELIGIBLE = [
    ("k = 100: not in 8-k blocks", dict(k=100)),
    ("k = 56: below a chunk", dict(k=56)),
    ("k = 128: whole chunks", dict(k=128)),
    ("bf16", dict(dt=BF16)),
    ("the generic kernel forced", dict(force=8)),
    ("m and n ragged with the edge tiles off", dict(m=129, n=260)),
]


@pytest.mark.parametrize("what,call", INELIGIBLE, ids=[c[0].split(":")[0] for c in INELIGIBLE])
def test_ineligible_calls_are_untouched(rt, what, call):
    kw = dict(m=128, n=256, k=200)
    kw.update(call)
    m, n, k, dt = kw.pop("m"), kw.pop("n"), kw.pop("k"), kw.get("dt", F32)
    A, B, C, D = operands(m, n, k, 1, 11)
    if dt == BF16:
        A, B, C, D = (orc.f32_to_bf16(x) for x in (A, B, C, D))
    before = (rt.edge_k_stats(), rt.edge_tiles_stats())
    want, want_refined = layer_call(rt, m, n, k, 1, A, B, C, D, **kw)
    for mode in (1, 6, 9):
        rt.set_edge_k(mode)
        got, refined = layer_call(rt, m, n, k, 1, A, B, C, D, **kw)
        assert refined == want_refined and "ragged k" not in refined, (what, mode, refined, want_refined)
        assert np.array_equal(ed.bits(got), ed.bits(want)), (what, mode)
    assert (rt.edge_k_stats(), rt.edge_tiles_stats()) == before, what


@pytest.mark.parametrize("variant", [6, 7, 9, 10])
def test_host_pointers(rt, variant):
    bm, bn = TILE[variant]
    exact_call(rt, variant, 2 * bm, 2 * bn, 168, 3, "beta1_bias_relu", variant, edge=False, mode="host")
    exact_call(rt, variant, bm + 1, bn + 4, 96, 1, "beta1_bias_relu", variant, edge=True, mode="host")


def test_a_replayed_tile_queue_group_is_untouched(rt):
    """64x64x96 items through the tile queue: what the queue groups is planned by plan_gemm_group, which knows no ragged-k mode"""
    import torch
    tm, tn, tk, MB, NB, KB = 64, 64, 96, 4, 6, 2
    rng = np.random.default_rng(8)
    X = rng.uniform(-1, 1, MB * KB * tm * tk).astype(np.float32)
    W = rng.uniform(-0.3, 0.3, NB * KB * tk * tn).astype(np.float32)
    C0 = rng.uniform(-1, 1, MB * NB * tm * tn).astype(np.float32)
    h = rt.brgemm_dispatch(F32, tm, tn, tk, tk, tn, tn, tm * tk, tk * tn, 0)
    dX, dW = torch.from_numpy(X).cuda(), torch.from_numpy(W).cuda()
    before = (rt.edge_k_stats(), rt.edge_tiles_stats())
    grouped_before = rt.tile_queue_stats()[0]
    prev_async, prev_q = rt.set_async(True), rt.set_tile_queue(1)
    results = {}
    try:
        for mode in (0, 1, 9):
            rt.set_edge_k(mode)
            for rep in range(3):  # recorded, then replayed
                dC = torch.from_numpy(C0.copy()).cuda()
                rt.synchronize()
                for i in range(MB):
                    for j in range(NB):
                        rt.brgemm(F32, h, dX, i * KB * tm * tk, dW, j * KB * tk * tn, dC, (i * NB + j) * tm * tn, KB)
                rt.synchronize()
                results[(mode, rep)] = (rt.last_grouped_kernel(), digest(dC.cpu().numpy()))
    finally:
        rt.set_edge_k(0)
        rt.synchronize()
        rt.set_tile_queue(prev_q)
        rt.set_async(prev_async)
    assert rt.tile_queue_stats()[0] > grouped_before, "the items were not grouped"
    for mode in (1, 9):
        for rep in range(3):
            assert results[(mode, rep)] == results[(0, rep)], (mode, rep, results)
    assert (rt.edge_k_stats(), rt.edge_tiles_stats()) == before
