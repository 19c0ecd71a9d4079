"""bf16 edge tiles (include/tpp_xsmm_abi.h xsmm_hip_set_edge_tiles, modes 2 and 20 .. 23) on a real MI355X: a whole-layer bf16 call whose m
or n no loader-wave tile divides runs on ceil(m / BM) x ceil(n / BN) workgroups of brgemm_bf16_lw - the last tile of a row or column of
tiles shifted back inside the matrix, storing only the rows and 16-byte pieces no other tile owns.

For a tile (bm, bn) the shapes are m in {bm + 1, 2 bm - 1, 3 bm + 17} x n in {bn + 8, 2 bn - 8, 3 bn + 24} - an overlap of all but one row /
one 16-byte piece, of one row / piece, several interior tiles with one ragged edge each way - plus m ragged with n divisible and the
reverse; k = 64 with 1, 2, 5 and 10 batch elements: one chunk, an even count (the two-chunks-per-barrier instances of 32x64 + K2 and
64x64), odd and more than the 4-slot ring, more than the 8-slot ring.
  1 exact inputs (tests/exact_data.py), bit for bit against the oracle: modes 20 .. 23, the three B images, four epilogues, one of them
    with poisoned memory around every operand and the output; then the reported kernel and the four counters
  2 random operands: the m x n window has the bits the same forced tile gives on the shape padded up to whole tiles; rows and columns of C
    beyond the window untouched; within one bf16 ulp of the oracle
  3 more tiles than can be resident, beta = 1 + bias: three runs, each the oracle's bits
  4 mode 2: the reported tile is the rule's (tests/test_gemm_plan_edge_bf16.py edge_rule = tests/golden/gemm_plan_edge_bf16.txt); an f32
    ragged call under mode 2 reports what it reports under mode 1
  5 ineligible calls: the kernel and the bits of mode 0, the counters do not move; modes 1 and 6 leave bf16 alone
  6 host pointers   7 strict mode, in a process of its own   8 xsmm_hip_fused_brgemm_chain_invoke on ragged layers: call by call, on edge
  tiles   9 a replayed tile-queue group of 64x48x64 items is untouched
Every case resets the mode to 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from edge_tiles_bf16_worker import BF16, VB, b_image, digest, layer_call, operands
from oracle import pyoracle as orc
from test_gemm_plan_edge_bf16 import edge_rule
from test_parity_gpu import F32, check_close, dev, gemm_case

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]  # mode 20 + t -> output tile
TILE_NAME = ["<32x64,k2>", "<64x64>", "<64x128>", "<128x128>"]
FAMILY = {2: "brgemm_bf16_lw", 0: "brgemm_bf16_lw_flatb", 4: "brgemm_bf16_lw_vnni4"}  # B image -> kernel family
BASE = {2: 20, 0: 24, 4: 28}                                                           # ... -> GemmVariant of its 32x64 + K2 tile


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def shapes(t):
    bm, bn = TILE[t]
    ms, ns = (bm + 1, 2 * bm - 1, 3 * bm + 17), (bn + 8, 2 * bn - 8, 3 * bn + 24)
    return [(m, n) for m in ms for n in ns] + [(2 * bm + 5, 2 * bn), (2 * bm, 2 * bn + 8)]


def assert_edge_launch(rt, before, t, image, m, n):
    """the launch just made ran on edge tiles of tile t with B image `image`: the reported kernel, and the counters as computed from the shape"""
    refined, after = rt.last_refined_kernel(), rt.edge_tiles_stats()
    assert refined == FAMILY[image] + TILE_NAME[t] + ", edge tiles", refined
    bm, bn = TILE[t]
    assert after == (before[0] + 1, -(-m // bm), -(-n // bn), BASE[image] + t), (before, after, m, n)


EPILOGUES = {"beta0": dict(beta0=True), "beta1_bias_relu": dict(bias=True, relu=True),
             "strided": dict(beta0=True, bias=True, strided=True), "poison": dict(beta0=True, bias=True, relu=True, strided=True, poison=True)}


def exact_call(rt, t, image, m, n, br, ep, seed, mode="device"):
    """gemm_case on exact inputs with the edge-tile mode already set: bit for bit the oracle's, nothing written outside the m x n window
    (with poison: and nothing read outside the operand windows); then the kernel and the counters"""
    kw = dict(EPILOGUES[ep])
    K = 64 * br
    if kw.pop("strided", False):  # leading dimensions beyond the rows, every base pointer moved: A, B, C by 16 bytes, the bias row by 8
        kw.update(lda=K + 8, ldb=n + 8, ldc=n + 16, sb=64 * (n + 8), offs=(8, 16, 8, 4))
    else:
        kw.update(lda=K, ldb=n, sb=64 * n)
    before = rt.edge_tiles_stats()
    with b_image(rt, image):
        gemm_case(rt, BF16, m, n, 64, br, sa=64, vnni=bool(image), values="exact", ranges=ed.exact_ranges(BF16, K), seed=seed, mode=mode, **kw)
    assert_edge_launch(rt, before, t, image, m, n)


@pytest.mark.parametrize("br", [1, 2, 5, 10])
@pytest.mark.parametrize("ep", sorted(EPILOGUES))
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_exact_inputs_bit_for_bit_against_the_oracle(rt, t, image, ep, br):
    assert rt.set_edge_tiles(20 + t) == 0
    try:
        for i, (m, n) in enumerate(shapes(t)):
            exact_call(rt, t, image, m, n, br, ep, 1000 * t + 100 * image + 10 * i + br)
    finally:
        rt.set_edge_tiles(0)


@pytest.mark.parametrize("which", [0, 4, 8, 9, 10])
@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_random_operands_have_the_bits_of_the_padded_shape(rt, t, image, which):
    """an element's chain of additions does not depend on where its tile sits: the ragged call under the mode against the same forced
    tile, mode 0, on the shape padded up to whole tiles - the same A, B and bias buffers, an equal copy of C (beta = 1 + bias + relu)"""
    m, n = shapes(t)[which]
    bm, bn = TILE[t]
    Mp, Np, K = -(-m // bm) * bm, -(-n // bn) * bn, 320
    A, B, C, D = operands(Mp, Np, K, 31 * t + 7 * image + which)
    before = rt.edge_tiles_stats()
    try:
        assert rt.set_edge_tiles(20 + t) == 0
        got, refined = layer_call(rt, image, m, n, K, A, B, C, D, ldb=Np, ldc=Np)
        assert_edge_launch(rt, before, t, image, m, n)
        rt.set_edge_tiles(0)
        padded, refined_padded = layer_call(rt, image, Mp, Np, K, A, B, C, D, force=BASE[image] + t)
    finally:
        rt.set_edge_tiles(0)
    assert refined_padded == "" and rt.edge_tiles_stats()[0] == before[0] + 1
    g, p, c = (x[:Mp * Np].reshape(Mp, Np) for x in (got, padded, C))
    assert np.array_equal(g[:m, :n], p[:m, :n]), "%d of %d elements differ from the padded launch" % (int((g[:m, :n] != p[:m, :n]).sum()), m * n)
    assert np.array_equal(g[m:, :], c[m:, :]) and np.array_equal(g[:, n:], c[:, n:]), "wrote beyond the m x n window"
    assert np.array_equal(got[Mp * Np:], C[Mp * Np:])
    ref = C.copy()
    with b_image(rt, image):
        orc.fused_brgemm(BF16, m, n, 64, K, Np, Np, 64, 64 * Np, VB if image else 0, 0, 5, 4, 1, A, 0, B, 0, ref, 0, D, 0, K // 64)
    win = lambda x: x[:Mp * Np].reshape(Mp, Np)[:m, :n]  # noqa: E731
    check_close(win(got), win(ref), BF16, "bf16 edge tiles %s m%d n%d K%d" % (refined, m, n, K))


def crowded_shape(t):
    """ragged both ways, 17 tile rows, and more tiles than the chip holds at once (these tiles run one workgroup per CU)"""
    bm, bn = TILE[t]
    need = cu_count() + 1
    tn = -(-need // 17)
    return 16 * bm + 1, (tn - 1) * bn + 8, 17 * tn, need


@pytest.mark.parametrize("t", [0, 3])
def test_more_tiles_than_can_be_resident_beta_1(rt, t):
    """tiles of a later round start after neighbours of an earlier one have stored: a tile that stored where it does not own C - or kept
    for itself what it read there - would show. Each of the three runs must be the oracle's bits (and so all three the same)"""
    m, n, tiles, need = crowded_shape(t)
    assert tiles >= need
    assert rt.set_edge_tiles(20 + t) == 0
    try:
        for _ in range(3):
            before = rt.edge_tiles_stats()
            gemm_case(rt, BF16, m, n, 64, 1, lda=64, ldb=n, sa=64, sb=64 * n, bias=True, vnni=True, values="exact", ranges=ed.exact_ranges(BF16, 64), seed=t)
            assert_edge_launch(rt, before, t, 2, m, n)
    finally:
        rt.set_edge_tiles(0)


@pytest.mark.parametrize("m,n", [(1000, 1000), (200, 1000), (4100, 1024)])
def test_mode_2_takes_the_tile_of_the_table(rt, m, n):
    t = edge_rule(m, n, 1, 2, cu_count())
    if cu_count() == 256:  # tests/golden/gemm_plan_edge_bf16.txt, the br1 cus256 rows
        assert t == {(1000, 1000): 1, (200, 1000): 0, (4100, 1024): 3}[(m, n)]
    assert rt.set_edge_tiles(2) == 0
    try:
        exact_call(rt, t, 2, m, n, 1, "beta1_bias_relu", m + n)
    finally:
        rt.set_edge_tiles(0)


def test_mode_2_is_mode_1_for_an_f32_call(rt):
    from edge_tiles_worker import layer_call as f32_call, operands as f32_operands
    A, B, C, D = f32_operands(200, 1000, 128, 5)
    seen = {}
    try:
        for mode in (1, 2, 21):
            assert rt.set_edge_tiles(mode) == 0
            before = rt.edge_tiles_stats()
            got, refined = f32_call(rt, 200, 1000, 128, A, B, C, D)
            after = rt.edge_tiles_stats()
            seen[mode] = (refined, after[0] - before[0], after[1:] if after[0] != before[0] else None, digest(got.view(np.uint16)))
            rt.set_edge_tiles(0)
    finally:
        rt.set_edge_tiles(0)
    assert seen[2] == seen[1] and seen[1][0].endswith(", edge tiles") and seen[1][1] == 1, seen
    assert "edge" not in seen[21][0] and seen[21][1] == 0, seen


# (what, modes, call): everything else about the call is eligible - m = 100, n = 200, K = 128, a VNNI-2 B, 16-byte aligned
INELIGIBLE = [
    ("m = 31: below every tile", (2, 20, 21), dict(m=31)),
    ("m = 63: below the 64-row tiles", (21, 22, 23), dict(m=63)),
    ("n = 68: no 16-byte pieces", (2, 21), dict(n=68, ldb=72, ldc=72)),
    ("k = 96: no 64-k chunks", (2, 21), dict(k=96, K=96)),
    ("A off its 16 bytes", (2, 21), dict(offs=(4, 0, 0, 0))),
    ("ldc not a multiple of 8", (2, 21), dict(ldc=204)),
    ("the bias row off its 8 bytes", (2, 21), dict(offs=(0, 0, 0, 2))),
    ("a VNNI C", (2, 21), dict(vnni_c=True)),
    ("the generic kernel forced", (2, 21), dict(force=8)),
    ("a divisible shape", (2, 20, 21, 22, 23), dict(m=128, n=256)),
    ("modes 1 and 6 leave bf16 alone", (1, 6), dict()),
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
        want, want_refined = layer_call(rt, 2, m, n, K, A, B, C, D, **kw)
        for mode in modes:
            assert rt.set_edge_tiles(mode) == 0
            got, refined = layer_call(rt, 2, m, n, K, A, B, C, D, **kw)
            rt.set_edge_tiles(0)
            assert refined == want_refined and "edge" not in refined, (what, mode, refined, want_refined)
            assert np.array_equal(got, want), (what, mode)
    finally:
        rt.set_edge_tiles(0)
    assert rt.edge_tiles_stats() == before, what


def test_the_setter_takes_the_documented_modes_only(rt):
    try:
        for mode in (2, 20, 21, 22, 23, 1, 6, 7, 9, 10):
            assert rt.set_edge_tiles(mode) == 0 and rt.set_edge_tiles(0) == mode
        for mode in (-1, 3, 5, 8, 11, 19, 24, 28, 31):
            assert rt.set_edge_tiles(mode) == -1 and rt.set_edge_tiles(0) == 0
    finally:
        rt.set_edge_tiles(0)


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_host_pointers(rt, t, image):
    m, n = shapes(t)[8]
    assert rt.set_edge_tiles(20 + t) == 0
    try:
        exact_call(rt, t, image, m, n, 5, "beta1_bias_relu", t, mode="host")
    finally:
        rt.set_edge_tiles(0)


@pytest.mark.parametrize("t,image", [(1, 2), (3, 0)])
def test_strict_mode_same_kernel_same_bits(rt, t, image):
    m, n = shapes(t)[8]
    bm, bn = TILE[t]
    K = 192
    A, B, C, D = operands(m, n, K, 40 + t)
    before = rt.edge_tiles_stats()
    try:
        assert rt.set_edge_tiles(20 + t) == 0
        got, refined = layer_call(rt, image, m, n, K, A, B, C, D)
        assert_edge_launch(rt, before, t, image, m, n)
    finally:
        rt.set_edge_tiles(0)
    # strict mode is chosen before anything is queued: a fresh child process (the mode arrives through the environment there)
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_STRICT", "TPP_HIP_EDGE_TILES", "TPP_HIP_TAIL_SPLIT", "TPP_HIP_SPLIT", "TPP_HIP_VNNI_FACTOR")}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_EDGE_TILES=str(20 + t))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edge_tiles_bf16_worker.py")] + [str(x) for x in (20 + t, image, m, n, K, 40 + t)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["edge_tiles_from_env"] == 20 + t
    assert d["kernels"] == [refined] * 3, d["kernels"]
    assert d["stats"] == [3, -(-m // bm), -(-n // bn), BASE[image] + t]
    assert set(d["digests"]) == {digest(got)}, "strict mode takes the same decision: the same bits"


@pytest.mark.parametrize("mode", [2, 21])
def test_chain_invoke_of_ragged_layers_runs_call_by_call_on_edge_tiles(rt, mode):
    """three bf16 VNNI-2 layers, m = 200, n = k = 128: no chain launch takes them (chains know no edge tiles), so the runtime runs them
    call by call - and each call is an edge launch. The bits are those of the three calls made one by one"""
    import torch
    m, w, br = 200, 128, 2
    rng = np.random.default_rng(3)
    X = orc.f32_to_bf16(rng.uniform(-1, 1, m * w).astype(np.float32))
    Ws = [orc.f32_to_bf16(rng.uniform(-0.2, 0.2, w * w).astype(np.float32)) for _ in range(3)]
    Ds = [orc.f32_to_bf16(rng.uniform(-1, 1, w).astype(np.float32)) for _ in range(3)]
    h = rt.fused_brgemm_dispatch(BF16, m, w, 64, w, w, w, 64, 64 * w, 4 | VB, 0, 5, 4, 1)
    dW, dD = [dev(x) for x in Ws], [dev(x) for x in Ds]

    def buffers():
        return [dev(X)] + [torch.zeros(m * w, dtype=torch.int16, device="cuda") for _ in range(3)]
    try:
        assert rt.set_edge_tiles(mode) == 0
        one = buffers()
        before = rt.edge_tiles_stats()
        for l in range(3):
            rt.fused_brgemm(BF16, h, one[l], 0, dW[l], 0, one[l + 1], 0, dD[l], 0, br)
            assert rt.last_refined_kernel().endswith(", edge tiles")
        rt.synchronize()
        assert rt.edge_tiles_stats()[0] == before[0] + 3
        ch = buffers()
        before = rt.edge_tiles_stats()
        ran_as_one = rt.fused_brgemm_chain(BF16, [(h, ch[l], 0, dW[l], 0, ch[l + 1], 0, dD[l], 0, br) for l in range(3)])
        rt.synchronize()
        assert not ran_as_one, "xsmm_hip_fused_brgemm_chain_invoke returns 0: call by call"
        assert rt.edge_tiles_stats()[0] == before[0] + 3
    finally:
        rt.set_edge_tiles(0)
    for l in range(1, 4):
        assert np.array_equal(ch[l].cpu().numpy(), one[l].cpu().numpy()), "layer %d" % l
    assert np.abs(orc.bf16_to_f32(one[3].cpu().numpy().view(np.uint16))).max() > 0


def test_a_replayed_tile_queue_group_is_untouched(rt):
    """--tiles=64,48,64 bf16 items through the tile queue: what the queue groups is planned by plan_gemm_group, which knows no edge tiles"""
    tm, tn, tk, MB, NB, KB = 64, 48, 64, 4, 6, 2
    rng = np.random.default_rng(8)
    X = orc.f32_to_bf16(rng.uniform(-1, 1, MB * KB * tm * tk).astype(np.float32))
    W = orc.f32_to_bf16(rng.uniform(-0.3, 0.3, NB * KB * tk * tn).astype(np.float32))
    C0 = orc.f32_to_bf16(rng.uniform(-1, 1, MB * NB * tm * tn).astype(np.float32))
    h = rt.brgemm_dispatch(BF16, tm, tn, tk, tk, tn, tn, tm * tk, tk * tn, VB)
    dX, dW = dev(X), dev(W)
    before = rt.edge_tiles_stats()
    prev_async, prev_q = rt.set_async(True), rt.set_tile_queue(1)
    results = {}
    try:
        for mode in (0, 2, 21):
            rt.set_edge_tiles(mode)
            for rep in range(3):  # recorded, then replayed
                dC = dev(C0)
                rt.synchronize()
                for i in range(MB):
                    for j in range(NB):
                        rt.brgemm(BF16, h, dX, i * KB * tm * tk, dW, j * KB * tk * tn, dC, (i * NB + j) * tm * tn, KB)
                rt.synchronize()
                results[(mode, rep)] = (rt.last_grouped_kernel(), digest(dC.cpu().numpy().view(np.uint16)))
    finally:
        rt.set_edge_tiles(0)
        rt.synchronize()
        rt.set_tile_queue(prev_q)
        rt.set_async(prev_async)
    assert results[(0, 2)][0] != "", "the items were not grouped"
    for mode in (2, 21):
        for rep in range(3):
            assert results[(mode, rep)] == results[(0, rep)], (mode, rep, results)
    assert rt.edge_tiles_stats() == before
