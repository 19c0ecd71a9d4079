"""Edge tiles (include/tpp_xsmm_abi.h xsmm_hip_set_edge_tiles) on a real MI355X: a whole-layer f32 call whose m or n no loader-wave tile
divides runs on ceil(m / BM) x ceil(n / BN) workgroups of brgemm_f32_lw_edge - the last tile of a row or column of tiles shifted back
inside the matrix, storing only what no other tile owns.

For a tile (bm, bn) the shapes are m in {bm + 1, 2 bm - 1, 3 bm + 17} x n in {bn + 4, 2 bn - 4, 3 bn + 20} - an overlap of all but one
row, of one row, several interior tiles with one ragged edge each way - plus m ragged with n divisible and the reverse; k = 64 with 1, 3
and 5 batch elements: a single chunk, fewer chunks than ring slots, more.
  1 exact inputs (tests/exact_data.py), bit for bit against the oracle: modes 6, 7, 9, 10, four epilogues, one of them with poisoned
    memory around every operand and the output
  2 random operands: the m x n window has the bits the same forced tile gives on the shape padded up to whole tiles; rows and columns of C
    beyond the window untouched; within the f32 bars against the oracle
  3 more tiles than can be resident, beta = 1: three runs, each the oracle's bits
  4 mode 1: the reported tile is the rule's (tests/test_gemm_plan_edge.py edge_rule = tests/golden/gemm_plan_edge.txt)
  5 ineligible calls: the kernel and the bits of mode 0, the counters do not move
  6 host pointers   7 strict mode, in a process of its own   8 a replayed tile-queue group of 64x48x64 items is untouched
Every case resets the mode to 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from edge_tiles_worker import digest, layer_call, operands
from oracle import pyoracle as orc
from test_gemm_plan_edge import edge_rule
from test_parity_gpu import F32, check_close, gemm_case

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = {6: (64, 64), 7: (64, 32), 9: (32, 32), 10: (128, 64)}  # mode = GemmVariant -> output tile
NAME = {6: "brgemm_f32_lw<64x64,k2>", 7: "brgemm_f32_lw<64x32,k4>", 9: "brgemm_f32_lw<32x32,k4>", 10: "brgemm_f32_lw<128x64,k1>"}


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def shapes(variant):
    bm, bn = TILE[variant]
    ms, ns = (bm + 1, 2 * bm - 1, 3 * bm + 17), (bn + 4, 2 * bn - 4, 3 * bn + 20)
    return [(m, n) for m in ms for n in ns] + [(2 * bm + 5, 2 * bn), (2 * bm, 2 * bn + 8)]


def assert_edge_launch(rt, before, variant, m, n):
    """the launch just made ran on edge tiles of `variant`: the reported kernel, and the counters as computed from the shape"""
    refined, after = rt.last_refined_kernel(), rt.edge_tiles_stats()
    assert refined == NAME[variant] + ", edge tiles", refined
    bm, bn = TILE[variant]
    assert after == (before[0] + 1, -(-m // bm), -(-n // bn), variant), (before, after, m, n)


EPILOGUES = {"beta0": dict(beta0=True), "beta1_bias_relu": dict(bias=True, relu=True),
             "strided": dict(beta0=True, bias=True, strided=True), "poison": dict(beta0=True, bias=True, relu=True, strided=True, poison=True)}


def exact_call(rt, variant, m, n, br, ep, seed, mode="device"):
    """gemm_case on exact inputs under edge-tile mode `variant`: bit for bit the oracle's, nothing written outside the m x n window (with
    poison: and nothing read outside the operand windows); then the kernel and the counters"""
    kw = dict(EPILOGUES[ep])
    K = 64 * br
    if kw.pop("strided", False):
        kw.update(lda=K + 8, ldb=n + 4, ldc=n + 4, sb=64 * (n + 4), offs=(4, 8, 4, 4))
    else:
        kw.update(lda=K, ldb=n, sb=64 * n)
    before = rt.edge_tiles_stats()
    gemm_case(rt, F32, m, n, 64, br, sa=64, values="exact", ranges=ed.exact_ranges(F32, K), seed=seed, mode=mode, **kw)
    assert_edge_launch(rt, before, variant, m, n)


@pytest.mark.parametrize("br", [1, 3, 5])
@pytest.mark.parametrize("ep", sorted(EPILOGUES))
@pytest.mark.parametrize("variant", [6, 7, 9, 10])
def test_exact_inputs_bit_for_bit_against_the_oracle(rt, variant, ep, br):
    assert rt.set_edge_tiles(variant) == 0
    try:
        for i, (m, n) in enumerate(shapes(variant)):
            exact_call(rt, variant, m, n, br, ep, 1000 * variant + 10 * i + br)
    finally:
        rt.set_edge_tiles(0)


def oracle_layer(m, n, K, lda, ldb, ldc, A, B, C, D):
    """beta = 1 + bias + relu: the result and |C| + sum |a||b| + |bias|"""
    ref, mag = C.copy(), np.abs(C)
    orc.fused_brgemm(F32, m, n, 64, lda, ldb, ldc, 64, 64 * ldb, 0, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, K // 64)
    orc.fused_brgemm(F32, m, n, 64, lda, ldb, ldc, 64, 64 * ldb, 0, 0, 0, 4, 1, np.abs(A), 0, np.abs(B), 0, mag, 0, np.abs(D), 0, K // 64)
    return ref, mag


@pytest.mark.parametrize("which", [0, 4, 8, 9, 10])
@pytest.mark.parametrize("variant", [6, 7, 9, 10])
def test_random_operands_have_the_bits_of_the_padded_shape(rt, variant, which):
    """an element's chain of additions does not depend on where its tile sits: the ragged call under the mode against the same forced
    tile, mode 0, on the shape padded up to whole tiles - the same A, B and bias buffers, an equal copy of C"""
    m, n = shapes(variant)[which]
    bm, bn = TILE[variant]
    Mp, Np, K = -(-m // bm) * bm, -(-n // bn) * bn, 320
    A, B, C, D = operands(Mp, Np, K, 31 * variant + which)
    before = rt.edge_tiles_stats()
    try:
        assert rt.set_edge_tiles(variant) == 0
        got, refined = layer_call(rt, m, n, K, A, B, C, D, ldb=Np, ldc=Np)
        assert_edge_launch(rt, before, variant, m, n)
        rt.set_edge_tiles(0)
        padded, refined_padded = layer_call(rt, Mp, Np, K, A, B, C, D, force=variant)
    finally:
        rt.set_edge_tiles(0)
    assert refined_padded == "" and rt.edge_tiles_stats()[0] == before[0] + 1
    g, p, c = (x[:Mp * Np].reshape(Mp, Np).view(np.uint32) for x in (got, padded, C))
    assert np.array_equal(g[:m, :n], p[:m, :n]), "%d of %d elements differ from the padded launch" % (int((g[:m, :n] != p[:m, :n]).sum()), m * n)
    assert np.array_equal(g[m:, :], c[m:, :]) and np.array_equal(g[:, n:], c[:, n:]), "wrote beyond the m x n window"
    assert np.array_equal(got[Mp * Np:].view(np.uint32), C[Mp * Np:].view(np.uint32))
    ref, mag = oracle_layer(m, n, K, K, Np, Np, A, B, C, D)
    win = lambda x: x[:Mp * Np].reshape(Mp, Np)[:m, :n]  # noqa: E731
    check_close(win(got), win(ref), F32, "edge tiles %s m%d n%d K%d" % (refined, m, n, K), win(mag), K)


def crowded_shape(variant):
    """ragged both ways, 17 tile rows, and more tiles than the chip holds at once: 32x32 + K4 workgroups run two per CU (64 KiB of LDS each),
    the 64-row tiles one"""
    bm, bn = TILE[variant]
    need = (2 if variant == 9 else 1) * cu_count() + 1
    tn = max(-(-need // 17), 2)
    return 16 * bm + 1, (tn - 1) * bn + 4, 17 * tn, need


@pytest.mark.parametrize("variant", [6, 9])
def test_more_tiles_than_can_be_resident_beta_1(rt, variant):
    """tiles of a later round start after neighbours of an earlier one have stored: a tile that joined C where it does not own it, or
    stored there, would show. Each of the three runs must be the oracle's bits (and so all three the same)"""
    m, n, tiles, need = crowded_shape(variant)
    assert tiles >= need
    assert rt.set_edge_tiles(variant) == 0
    try:
        for _ in range(3):
            before = rt.edge_tiles_stats()
            gemm_case(rt, F32, m, n, 64, 1, lda=64, ldb=n, sa=64, sb=64 * n, bias=True, values="exact", ranges=ed.exact_ranges(F32, 64), seed=variant)
            assert_edge_launch(rt, before, variant, m, n)
    finally:
        rt.set_edge_tiles(0)


@pytest.mark.parametrize("m,n", [(1000, 1000), (200, 1000), (4000, 520)])
def test_mode_1_takes_the_tile_of_the_table(rt, m, n):
    variant = edge_rule(m, n, 1, cu_count())
    if cu_count() == 256:  # tests/golden/gemm_plan_edge.txt, cus256 rows
        assert variant == {(1000, 1000): 6, (200, 1000): 9, (4000, 520): 6}[(m, n)]
    assert rt.set_edge_tiles(1) == 0
    try:
        exact_call(rt, variant, m, n, 1, "beta1_bias_relu", m + n)
    finally:
        rt.set_edge_tiles(0)


# (what, modes, call): everything else about the call is eligible - m = 100, n = 200, K = 128 row-major, 16-byte aligned
INELIGIBLE = [
    ("m = 63: below the 64-row tiles", (6, 7, 10), dict(m=63)),
    ("m = 31: below every tile", (1, 6), dict(m=31)),
    ("n = 70: no 16-byte pieces", (1, 6), dict(n=70, ldb=72, ldc=72)),
    ("k = 96: no 64-k chunks", (1, 6), dict(k=96, K=96)),
    ("A one element off its 16 bytes", (1, 6), dict(offs=(1, 0, 0, 0))),
    ("ldc not a multiple of 4", (1, 6), dict(ldc=202)),
    ("the bias row off its 16 bytes", (1, 6), dict(offs=(0, 0, 0, 2))),
    ("the generic kernel forced", (1, 6), dict(force=8)),
]


@pytest.mark.parametrize("what,modes,call", INELIGIBLE, ids=[c[0].split(":")[0] for c in INELIGIBLE])
def test_ineligible_calls_are_untouched(rt, what, modes, call):
    kw = dict(m=100, n=200, K=128)
    kw.update(call)
    m, n, K = kw.pop("m"), kw.pop("n"), kw.pop("K")
    A, B, C, D = operands(m, n, K, 11, lda=kw.get("lda"), ldb=kw.get("ldb"), ldc=kw.get("ldc"))
    before = rt.edge_tiles_stats()
    try:
        rt.set_edge_tiles(0)
        want, want_refined = layer_call(rt, m, n, K, A, B, C, D, **kw)
        for mode in modes:
            rt.set_edge_tiles(mode)
            got, refined = layer_call(rt, m, n, K, A, B, C, D, **kw)
            assert refined == want_refined and "edge" not in refined, (what, mode, refined, want_refined)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, mode)
    finally:
        rt.set_edge_tiles(0)
    assert rt.edge_tiles_stats() == before, what


def test_m_63_under_mode_1_fits_the_32_row_tile(rt):
    """the tile rule's candidates are the tiles with m >= BM and n >= BN: m = 63 is ineligible for the 64-row tiles only"""
    assert edge_rule(63, 200, 1, cu_count()) == 9
    assert rt.set_edge_tiles(1) == 0
    try:
        exact_call(rt, 9, 63, 200, 2, "beta1_bias_relu", 63)
    finally:
        rt.set_edge_tiles(0)


@pytest.mark.parametrize("variant", [6, 7, 9, 10])
def test_host_pointers(rt, variant):
    m, n = shapes(variant)[8]
    assert rt.set_edge_tiles(variant) == 0
    try:
        exact_call(rt, variant, m, n, 3, "beta1_bias_relu", variant, mode="host")
    finally:
        rt.set_edge_tiles(0)


@pytest.mark.parametrize("variant", [6, 10])
def test_strict_mode_same_kernel_same_bits(rt, variant):
    m, n = shapes(variant)[8]
    bm, bn = TILE[variant]
    K = 192
    A, B, C, D = operands(m, n, K, 40 + variant)
    before = rt.edge_tiles_stats()
    try:
        assert rt.set_edge_tiles(variant) == 0
        got, refined = layer_call(rt, m, n, K, A, B, C, D)
        assert_edge_launch(rt, before, variant, m, n)
    finally:
        rt.set_edge_tiles(0)
    # strict mode is chosen before anything is queued: a fresh child process (the mode arrives through the environment there)
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_STRICT", "TPP_HIP_EDGE_TILES", "TPP_HIP_TAIL_SPLIT", "TPP_HIP_SPLIT")}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_EDGE_TILES=str(variant))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edge_tiles_worker.py")] + [str(x) for x in (variant, m, n, K, 40 + variant)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["edge_tiles_from_env"] == variant
    assert d["kernels"] == [refined] * 3, d["kernels"]
    assert d["stats"] == [3, -(-m // bm), -(-n // bn), variant]
    assert set(d["digests"]) == {digest(got)}, "strict mode takes the same decision: the same bits"


def test_a_replayed_tile_queue_group_is_untouched(rt):
    """--tiles=64,48,64 items through the tile queue: what the queue groups is planned by plan_gemm_group, which knows no edge tiles"""
    import torch
    tm, tn, tk, MB, NB, KB = 64, 48, 64, 4, 6, 2
    rng = np.random.default_rng(8)
    X = rng.uniform(-1, 1, MB * KB * tm * tk).astype(np.float32)
    W = rng.uniform(-0.3, 0.3, NB * KB * tk * tn).astype(np.float32)
    C0 = rng.uniform(-1, 1, MB * NB * tm * tn).astype(np.float32)
    h = rt.brgemm_dispatch(F32, tm, tn, tk, tk, tn, tn, tm * tk, tk * tn, 0)
    dX, dW = torch.from_numpy(X).cuda(), torch.from_numpy(W).cuda()
    before = rt.edge_tiles_stats()
    prev_async, prev_q = rt.set_async(True), rt.set_tile_queue(1)
    results = {}
    try:
        for mode in (0, 1, 9):
            rt.set_edge_tiles(mode)
            for rep in range(3):  # recorded, then replayed
                dC = torch.from_numpy(C0.copy()).cuda()
                rt.synchronize()
                for i in range(MB):
                    for j in range(NB):
                        rt.brgemm(F32, h, dX, i * KB * tm * tk, dW, j * KB * tk * tn, dC, (i * NB + j) * tm * tn, KB)
                rt.synchronize()
                results[(mode, rep)] = (rt.last_grouped_kernel(), digest(dC.cpu().numpy()))
    finally:
        rt.set_edge_tiles(0)
        rt.synchronize()
        rt.set_tile_queue(prev_q)
        rt.set_async(prev_async)
    assert results[(0, 2)][0] != "", "the items were not grouped"
    for mode in (1, 9):
        for rep in range(3):
            assert results[(mode, rep)] == results[(0, rep)], (mode, rep, results)
    assert rt.edge_tiles_stats() == before
