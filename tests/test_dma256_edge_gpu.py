"""Edge tiles on the 256x256 bf16 tile (include/tpp_xsmm_abi.h xsmm_hip_set_dma256_edge) on a real MI355X: with the switch on, a whole-layer
bf16 call with m, n >= 256 and m or n not a multiple of 256 runs on ceil(m / 256) x ceil(n / 256) workgroups of brgemm_bf16_dma256_edge /
_edge_flatb / _edge_vnni4; the last tile row and column are shifted back and store only what no other tile owns.

All cases run under mode 2 and leave the switch 0. m x n in {264x256 (two row tiles that overlap in 248 rows), 256x264 (two column tiles
that overlap in 248 columns), 520x776 (both ragged, 3 x 4 tiles, the linear grid), 1000x504 (4 x 2 tiles, the XCD-blocked grid)}; (k, br)
in {(32, 1) one chunk, (96, 1) the prologue only, (224, 1) one steady lap plus the tail, (64, 2) a batch with strides that are not the
packed ones}; B VNNI-2, flat and VNNI-4. Operands are strided (tests/dma256_images_worker.py Case): lda > k, ldb > n, ldc > n, every base
pointer moved, 8 guard rows / gap columns around every buffer - NaN around the inputs, a bit pattern around C, checked after every run.
  1 exact inputs, bit for bit the oracle's, beta 0 + bias + relu and beta 1 plain - after the case's own precondition: the oracle equals
    the fp64 result rounded once
  2 random operands, three steps on NaN-refilled outputs: the m x n window has the bits of the same elements of a LARGER problem that
    holds the call in its corner - an element's chain of additions does not depend on where its tile sits. Two larger problems:
    (a) every (k, br): rows and columns padded to the next multiple of 256 PLUS 8, on this kernel - the window's elements come from tiles
        that are not shifted there;
    (b) k % 64 == 0: padded to the next multiple of 256, switch off, on the divisible kernel - brgemm_bf16_dma<256x256> (forced variant
        18) for VNNI-2, under xsmm_hip_set_dma256_images(2) for flat and VNNI-4. The library runs that kernel on descriptors with k % 64
        == 0 only (gemm_plan.cpp bf16_fast_eligible, the loader-wave image tiles), so k = 32, 96 and 224 have no such reference: (a) and
        check 1 cover them.
    No tolerance: the same k values in the same order on the same MFMA with one rounding.
  3 every taken call asserts the reported kernel, the stats (count + 1, tile rows, tile columns, image) and that the edge-tile, edge-k
    and dma256-images counters stand still
  4 calls that stay where they are: the bits, the reported kernel and the stats of mode 0. The two-layer chain of a 264-row descriptor
    runs under xsmm_hip_set_chain_edge(1), as ONE chain launch: a chain the runtime runs call by call is, by its contract, those calls
  5 TPP_HIP_DMA256_EDGE=2 with TPP_HIP_STRICT=1 in a child process: the same launch, the same bits"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from dma256_edge_worker import BF16, Case, corner, digest, embedded, up256

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Case.image: 2 VNNI-2, 0 flat, 4 VNNI-4
TEXT = {2: "brgemm_bf16_dma<256x256>, edge tiles", 0: "brgemm_bf16_dma_flatb<256x256>, edge tiles", 4: "brgemm_bf16_dma_vnni4<256x256>, edge tiles"}
KIND = {2: 0, 0: 2, 4: 4}  # image -> what xsmm_hip_dma256_edge_stats reports
SHAPES = [(264, 256), (256, 264), (520, 776), (1000, 504)]
KBR = [(32, 1), (96, 1), (224, 1), (64, 2)]
IMAGES = [2, 0, 4]
EPS = (dict(beta0=True, bias=True, relu=True), dict(beta0=False, bias=False, relu=False))


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def mode_off(rt):
    rt.set_dma256_edge(0)
    yield
    rt.set_dma256_edge(0)


def other_counters(rt):
    return rt.edge_tiles_stats(), rt.edge_k_stats(), rt.edge_k_bf16_stats(), rt.edge_k8_bf16_stats(), rt.dma256_images_stats()


def run_taken(rt, case, mode=2):
    """the call under `mode`: it ran on the edge tiles with its image - the reported kernel, the counter moved by one, no other counter"""
    rt.set_dma256_edge(mode)
    before, others = rt.dma256_edge_stats(), other_counters(rt)
    got, refined, _ = case.run(rt)
    rt.set_dma256_edge(0)
    assert refined == TEXT[case.image], refined
    assert rt.dma256_edge_stats() == (before[0] + 1, -(-case.m // 256), -(-case.n // 256), KIND[case.image]), (before, rt.dma256_edge_stats())
    assert other_counters(rt) == others
    assert case.outside_untouched(got), "wrote outside the m x n window"
    return got


def run_stays(rt, case, mode, **kw):
    """the call under `mode` stays where it is: no edge tile of this switch reported, the counter still"""
    rt.set_dma256_edge(mode)
    before = rt.dma256_edge_stats()
    got, refined, name = case.run(rt, **kw)
    rt.set_dma256_edge(0)
    assert "<256x256>, edge tiles" not in refined and rt.dma256_edge_stats() == before, (refined, before, rt.dma256_edge_stats())
    return got, refined, name


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("image", IMAGES)
def test_exact_inputs_bit_for_bit_against_the_oracle_and_windows_intact(rt, image, m, n, k, br):
    for i, ep in enumerate(EPS):
        case = Case(image, m, n, k, br, 1000 * image + m + n + 10 * k + br + i, exact=True, **ep)
        ref = case.oracle()
        assert np.array_equal(ref[case.win], case.fp64()), "not an exact case: the oracle is not the fp64 result rounded once"
        assert case.outside_untouched(ref)
        got = run_taken(rt, case)
        ed.check_bits(got[case.win], ref[case.win], BF16, "%s m%d n%d k%d br%d %s" % (TEXT[image], m, n, k, br, sorted(x for x in ep if ep[x])))


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("image", IMAGES)
def test_random_operands_have_the_bits_of_the_padded_problem(rt, image, m, n, k, br):
    for i, ep in enumerate(EPS):
        seed = 77 * image + m + n + 10 * k + br + i
        what = "m%d n%d k%d br%d %s" % (m, n, k, br, sorted(x for x in ep if ep[x]))
        # (a) the corner of a larger ragged problem on this kernel: the window's tiles are not shifted there
        big = Case(image, up256(m) + 8, up256(n) + 8, k, br, seed, **ep)
        case = embedded(big, m, n, seed + 1)
        want = corner(big, run_taken(rt, big), m, n)
        assert np.isfinite(ed.as_f32(want)).all()
        for step in range(3):
            got = run_taken(rt, case)
            assert np.isfinite(ed.as_f32(got[case.win])).all(), "read poisoned memory"
            ed.check_bits(got[case.win], want, BF16, "%s against the corner of %d x %d, step %d: %s" % (TEXT[image], big.m, big.n, step, what))
        if k % 64:
            continue
        # (b) the corner of the problem padded to whole tiles on the divisible kernel, switch off
        pad = Case(image, up256(m), up256(n), k, br, seed + 2, **ep)
        case = embedded(pad, m, n, seed + 3)
        if image == 2:
            ref, _, name = run_stays(rt, pad, 0, force=18)
            assert name == "brgemm_bf16_dma<256x256>", name
        else:
            rt.set_dma256_images(2)
            try:
                ref, refined, _ = run_stays(rt, pad, 0)
            finally:
                rt.set_dma256_images(0)
            assert refined == ("brgemm_bf16_dma_vnni4<256x256>" if image else "brgemm_bf16_dma_flatb<256x256>"), refined
        want = corner(pad, ref, m, n)
        for step in range(3):
            got = run_taken(rt, case)
            ed.check_bits(got[case.win], want, BF16, "%s against the divisible kernel on %d x %d, step %d: %s" % (TEXT[image], pad.m, pad.n, step, what))


# (what, mode, how the eligible call - VNNI-2, 288 x 512, k = 64, br = 2 - differs)
STAYS = [
    ("mode 0", 0, dict()),
    ("a divisible 512 x 512 call", 2, dict(m=512)),
    ("m = 248", 2, dict(m=248)),
    ("n = 260", 2, dict(n=260)),
    ("k = 40", 2, dict(k=40)),
    ("a forced variant", 2, dict(force=20)),
]


@pytest.mark.parametrize("what,mode,kw", STAYS, ids=[s[0] for s in STAYS])
def test_calls_that_stay_where_they_are(rt, what, mode, kw):
    kw = dict(kw)
    force = kw.pop("force", None)
    case = Case(2, kw.pop("m", 288), kw.pop("n", 512), kw.pop("k", 64), 2, 5)
    want, off_kernel, _ = run_stays(rt, case, 0, force=force)
    got, refined, _ = run_stays(rt, case, mode, force=force)
    assert refined == off_kernel, (what, refined, off_kernel)
    assert np.array_equal(got, want), what
    if what == "mode 0":  # (and the same call IS taken under mode 2)
        run_taken(rt, case)


def test_an_f32_call_stays_where_it_is(rt):
    from edge_tiles_worker import layer_call as f32_call, operands as f32_operands
    A, B, C, D = f32_operands(264, 256, 128, 5)
    seen = {}
    for mode in (0, 2):
        rt.set_dma256_edge(mode)
        before = rt.dma256_edge_stats()
        got, refined = f32_call(rt, 264, 256, 128, A, B, C, D)
        rt.set_dma256_edge(0)
        assert rt.dma256_edge_stats() == before
        seen[mode] = (refined, digest(got.view(np.uint16)))
    assert seen[0] == seen[2], seen


def test_a_tile_queue_group_and_a_chain_stay_where_they_are(rt):
    """what is queued, grouped or chained never sees the switch: two queued invokes of a 64x64 tile descriptor (the tile queue takes tile
    invokes only), and two layers of a 264 x 256 x 256 descriptor - eligible as a single call - as one chain launch on edge row tiles
    (xsmm_hip_set_chain_edge). The counter still, the bits of mode 0"""
    case, tile = Case(2, 264, 256, 256, 1, 9, beta0=True, strided=False, poison=False), Case(2, 64, 64, 64, 1, 8, beta0=True, strided=False, poison=False)
    h, ht = case.dispatch(rt), tile.dispatch(rt)
    results = {}
    for mode in (0, 2):
        rt.set_dma256_edge(mode)
        before = rt.dma256_edge_stats()
        dA, dB, _, dD = case.device()
        tA, tB, _, tD = tile.device()
        outs = [tile.device()[2] for _ in range(2)] + [case.device()[2]]
        mid = case.device()[2]
        was_async, was_q, was_ce = rt.set_async(True), rt.set_tile_queue(1), rt.set_chain_edge(1)
        try:
            groups = rt.tile_queue_stats()[0]
            for o in outs[:2]:
                rt.fused_brgemm(BF16, ht, tA, 0, tB, 0, o, 0, tD, 0, 1)
            rt.flush()
            rt.synchronize()
            assert rt.tile_queue_stats()[0] > groups, "the two tile invokes did not run as a group"
            rt.set_tile_queue(0)
            ran = rt.fused_brgemm_chain(BF16, [(h, dA, 0, dB, 0, mid, 0, dD, 0, 1), (h, mid, 0, dB, 0, outs[2], 0, dD, 0, 1)])
            rt.synchronize()
            assert ran, "the 2-layer chain ran call by call"
        finally:
            rt.set_chain_edge(was_ce)
            rt.set_tile_queue(was_q)
            rt.set_async(was_async)
        assert rt.dma256_edge_stats() == before, (mode, before, rt.dma256_edge_stats())
        results[mode] = [digest(o.cpu().numpy()) for o in outs] + [digest(mid.cpu().numpy())]
    rt.set_dma256_edge(0)
    assert results[0] == results[2]
    # (and the same descriptor IS taken as a single call)
    run_taken(rt, case)


def test_the_environment_form_in_a_strict_child_process(rt):
    image, m, n, k, br, seed = 4, 520, 776, 64, 2, 21
    got = run_taken(rt, Case(image, m, n, k, br, seed))
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("TPP_HIP_")}
    env.update(TPP_HIP_DMA256_EDGE="2", TPP_HIP_STRICT="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dma256_edge_worker.py")] + [str(x) for x in (image, m, n, k, br, seed)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["from_env"] == 2 and d["strict"] == 1 and d["kernels"] == [TEXT[image]] * 3, d
    assert d["stats"] == [3, 3, 4, KIND[image]]
    assert set(d["digests"]) == {digest(got)}
