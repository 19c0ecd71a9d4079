"""Flat and VNNI-4 B on the 256x256 bf16 tile (include/tpp_xsmm_abi.h xsmm_hip_set_dma256_images) on a real MI355X: with the switch on, a
whole-layer bf16 call with a flat [k][ldb] or a VNNI-4 [k/4][ldb][4] B whose m and n the 256x256 tile divides runs on
brgemm_bf16_dma256_flatb / brgemm_bf16_dma256_vnni4 - the ring, A image, schedule and epilogue of brgemm_bf16_dma256, the B image of the operand.

All cases run under mode 2, so that these small shapes reach the kernel: m x n in {256x256 (one tile), 512x768 (the plain grid), 1024x512
(the XCD-blocked grid: tile rows % 4 == 0 and tile columns % 2 == 0)}; (k, br) in {(64, 1), (128, 1), (64, 3), (128, 2), (64, 7)} = 2, 4,
6, 8, 14 chunks of 32 k: below the three-chunk prologue, the tail alone, one steady lap plus tail, several laps. Operands are strided
(tests/dma256_images_worker.py Case): lda > k, ldb > n, ldc > n, batch strides that are not the packed ones, every base pointer moved.
  1 exact inputs, bit for bit the oracle's, beta 0 + bias + relu and beta 1 plain - after the case's own precondition: the oracle equals
    the fp64 result rounded once. NaN in the gap columns, between batch elements, in guard rows and in the beta-0 C window, a bit
    pattern around C: all intact
  2 random operands: bit for bit the same call with the mode off (the loader-wave tile: both kernels sum every output in one chain over
    k, in k order, on the same MFMA); a flat B also bit for bit its VNNI-2 pack on brgemm_bf16_dma<256x256>
  3 calls that stay where they are, the counter still   4 the setter; TPP_HIP_DMA256_IMAGES in a child process
Every case asserts the reported kernel and the counter, and leaves the mode 0."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from dma256_images_worker import BF16, Case, digest

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = {0: "brgemm_bf16_dma_flatb<256x256>", 4: "brgemm_bf16_dma_vnni4<256x256>"}
KIND = {0: 2, 4: 4}  # image -> what xsmm_hip_dma256_images_stats reports
SHAPES = [(256, 256), (512, 768), (1024, 512)]
KBR = [(64, 1), (128, 1), (64, 3), (128, 2), (64, 7)]
assert [k * br // 32 for k, br in KBR] == [2, 4, 6, 8, 14]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(autouse=True)
def mode_off(rt):
    rt.set_dma256_images(0)
    yield
    rt.set_dma256_images(0)


def run_taken(rt, case, mode=2):
    """the call under `mode`: it ran on the 256x256 tile with its image - the reported kernel, the counter moved by one"""
    rt.set_dma256_images(mode)
    before = rt.dma256_images_stats()
    got, refined, _ = case.run(rt)
    rt.set_dma256_images(0)
    assert refined == TEXT[case.image], refined
    assert rt.dma256_images_stats() == (before[0] + 1, case.m // 256, case.n // 256, KIND[case.image]), (before, rt.dma256_images_stats())
    return got


def run_stays(rt, case, mode, **kw):
    """the call under `mode` stays where it is: no such kernel reported, the counter still; returns the C buffer and the reported kernel"""
    rt.set_dma256_images(mode)
    before = rt.dma256_images_stats()
    got, refined, name = case.run(rt, **kw)
    rt.set_dma256_images(0)
    assert "brgemm_bf16_dma_" not in refined and rt.dma256_images_stats() == before, (refined, before, rt.dma256_images_stats())
    return got, refined, name


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("image", [0, 4])
def test_exact_inputs_bit_for_bit_against_the_oracle_and_windows_intact(rt, image, m, n, k, br):
    for i, ep in enumerate((dict(beta0=True, bias=True, relu=True), dict(beta0=False, bias=False, relu=False))):
        case = Case(image, m, n, k, br, 1000 * image + m + n + 10 * k + br + i, exact=True, **ep)
        ref = case.oracle()
        assert np.array_equal(ref[case.win], case.fp64()), "not an exact case: the oracle is not the fp64 result rounded once"
        assert case.outside_untouched(ref)
        got = run_taken(rt, case)
        ed.check_bits(got[case.win], ref[case.win], BF16, "%s m%d n%d k%d br%d %s" % (TEXT[image], m, n, k, br, sorted(x for x in ep if ep[x])))
        assert case.outside_untouched(got), "wrote outside the m x n window"


@pytest.mark.parametrize("k,br", KBR)
@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("image", [0, 4])
def test_random_operands_bit_for_bit_the_call_with_the_mode_off(rt, image, m, n, k, br):
    case = Case(image, m, n, k, br, 77 * image + m + n + 10 * k + br)
    # the mode-off side on the 128x128 image tile, where large calls run (these small shapes are planned on smaller tiles, and the 32x64
    # one splits k over two wave groups: two chains); a forced variant is never taken by the switch
    want, off_kernel, name = run_stays(rt, case, 2, force=31 if image else 27)
    assert name == "brgemm_bf16_lw_" + ("vnni4" if image else "flatb") + "<128x128>", name
    got = run_taken(rt, case)
    assert np.isfinite(ed.as_f32(got[case.win])).all(), "read poisoned memory"
    ed.check_bits(got[case.win], want[case.win], BF16, "%s against %s m%d n%d k%d br%d" % (TEXT[image], name, m, n, k, br))
    assert case.outside_untouched(got), "wrote outside the m x n window"
    if image == 0:  # the same B as VNNI-2 pair-rows on the kernel this one extends
        packed = case.as_vnni2()
        pk, _, pname = run_stays(rt, packed, 2, force=18)
        assert pname == "brgemm_bf16_dma<256x256>", pname
        ed.check_bits(got[case.win], pk[case.win], BF16, "flat B against its VNNI-2 pack on %s m%d n%d k%d br%d" % (pname, m, n, k, br))


STAYS = [
    ("mode 0", dict(mode=0)),
    ("mode 1 on a small shape", dict(mode=1)),
    ("m = 264", dict(m=264)),
    ("a VNNI-2 descriptor", dict(image=2)),
    ("a forced variant", dict(force=24)),
    ("a misaligned B", dict(offs=(8, 20, 8, 4))),
    ("an empty batch", dict(run_br=0)),
]


@pytest.mark.parametrize("what,kw", STAYS, ids=[s[0] for s in STAYS])
def test_calls_that_stay_where_they_are(rt, what, kw):
    kw = dict(kw)
    mode, force, run_br = kw.pop("mode", 2), kw.pop("force", None), kw.pop("run_br", None)
    case = Case(kw.pop("image", 0), kw.pop("m", 512), 256, 128, 2, 5, **kw)
    want, off_kernel, _ = run_stays(rt, case, 0, force=force, br=run_br)
    got, refined, _ = run_stays(rt, case, mode, force=force, br=run_br)
    assert refined == off_kernel, (what, refined, off_kernel)
    assert np.array_equal(got, want), what


def test_a_tile_queue_group_and_a_chain_stay_where_they_are(rt):
    """what is queued, grouped or chained never sees the switch. The tile queue takes tile invokes (up to 64x64) only - a descriptor the
    256x256 tile divides is never queued - so the group is four queued invokes of a flat-B 64x64 tile descriptor; the chain is two
    layers of an eligible 256x256 descriptor in one chain launch. The counter still, the bits of mode 0"""
    case, tile = Case(0, 256, 256, 256, 1, 9, beta0=True, strided=False, poison=False), Case(0, 64, 64, 64, 1, 8, beta0=True, strided=False, poison=False)
    h, ht = case.dispatch(rt), tile.dispatch(rt)
    results = {}
    for mode in (0, 2):
        rt.set_dma256_images(mode)
        before = rt.dma256_images_stats()
        dA, dB, _, dD = case.device()
        tA, tB, _, tD = tile.device()
        outs = [tile.device()[2] for _ in range(4)] + [case.device()[2]]
        mid = case.device()[2]
        was_async, was_q = rt.set_async(True), rt.set_tile_queue(1)
        try:
            groups = rt.tile_queue_stats()[0]
            for o in outs[:4]:
                rt.fused_brgemm(BF16, ht, tA, 0, tB, 0, o, 0, tD, 0, 1)
            rt.flush()
            rt.synchronize()
            assert rt.tile_queue_stats()[0] > groups, "the four tile invokes did not run as a group"
            rt.set_tile_queue(0)
            ran = rt.fused_brgemm_chain(BF16, [(h, dA, 0, dB, 0, mid, 0, dD, 0, 1), (h, mid, 0, dB, 0, outs[4], 0, dD, 0, 1)])
            rt.synchronize()
            assert ran, "the 2-layer chain ran call by call"
        finally:
            rt.set_tile_queue(was_q)
            rt.set_async(was_async)
        assert rt.dma256_images_stats() == before, (mode, before, rt.dma256_images_stats())
        results[mode] = [digest(o.cpu().numpy()) for o in outs] + [digest(mid.cpu().numpy())]
    rt.set_dma256_images(0)
    assert results[0] == results[2]
    # (and the same descriptor IS taken as a single call)
    run_taken(rt, case)


def test_the_setter_takes_0_1_2_only(rt):
    assert rt.set_dma256_images(1) == 0 and rt.set_dma256_images(2) == 1 and rt.set_dma256_images(0) == 2
    for bad in (-1, 3, 4, 20, 256):
        assert rt.set_dma256_images(bad) == -1 and rt.set_dma256_images(0) == 0
    assert len(rt.dma256_images_stats()) == 4


def test_the_environment_form_in_a_child_process(rt):
    image, m, n, k, br, seed = 4, 512, 768, 64, 3, 21
    got = run_taken(rt, Case(image, m, n, k, br, seed))
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("TPP_HIP_")}
    env.update(TPP_HIP_DMA256_IMAGES="2")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dma256_images_worker.py")] + [str(x) for x in (image, m, n, k, br, seed)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["from_env"] == 2 and d["kernels"] == [TEXT[image]] * 3, d
    assert d["stats"] == [3, m // 256, n // 256, KIND[image]]
    assert set(d["digests"]) == {digest(got)}
