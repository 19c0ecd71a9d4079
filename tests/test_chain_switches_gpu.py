"""ALL seven chain switches on at once, on a real MI355X: the configuration someone gets who turns on everything that pays. Every
tests/test_chain_*_gpu.py resets the other switches; tests/test_chain_dispatch.py shows on a CPU that the launch decision under any set of
switches is the decision of one of them alone. Here the same claim runs on the device: with xsmm_hip_set_chain_edge / _rounds / _ragged /
_widths / _width_rounds / _widths_ragged / _dma256 all at 1 (plus edge_tiles = 2, edge_k_bf16 = 1, edge_k8_bf16 = 1, dma256_images = 1), one
chain per launch form, at the smallest shape at which tests/golden/chain_dispatch.txt (rows 'dev ...', 256 compute units) shows the form:

  plain                64 rows x [64, 64, 64]             edge rows      100 rows x [128, 128, 128]
  ragged width         200 rows x [200] * 4               mixed widths   256 rows x [256, 512, 128, 256]
  ragged mixed widths  200 rows x [200, 136, 72, 200]     several rounds 64 * 257 rows x [64, 64, 64] (257 tiles of 64x64, the only tile that divides)
  256x256 tile         7680 rows x n = [2048, 2048], every k = 64 (30 x 8 tiles: the smallest VNNI-2 chain dispatched on that tile)
  column rounds        256 rows x [256, 512, 128, 256] with xsmm_hip_set_chain_width_rounds(1002): by rule no small chain shares a tile,
                       and a forced W is asked in front of the mixed-width rule (the table's D({wrounds}) is the rule's)
  refused everywhere   64 rows x [64, 100, 64] (n % 8 != 0)
(sizes: the input's width, then every layer's n; 32 * 257 rows, the issue's candidate for several rounds, runs on edge rows when both
switches are on - the table's row 'dev 8224x[64]*3'.) Buffers: chain_widths_worker.WidthsChain - 8 guard rows and 8 gap columns around
everything, NaN around the inputs and inside the outputs, a sentinel around them. Data is exact (small integers: every sum is exact in
f32 and every output in bf16), so every layer must be the oracle's bit for bit whatever tile or order computes it. B images: VNNI-2 and,
rotating over the cases, flat or VNNI-4. Per case, six steps on refilled outputs: every layer bit for bit the oracle's; nothing outside
the windows written; the *_stats counter that moved six times is the one the golden table names as D(all) for this chain and image (only
on a device of 256 compute units: the table's; otherwise the reason is printed and the check left out); no other chain counter moved;
and the same chain with every switch at 0 gives the same bits - include/tpp_xsmm_abi.h promises of xsmm_hip_fused_brgemm_chain_invoke
"exactly the effect of" the calls one by one and "Same arithmetic as the separate launches (f32 accumulation in k order, one rounding
per layer)", which on exact data is the same bits on any tile.
One further case alternates two chains whose counter-block keys coincide - 64 rows x [64] * 4 (plain) and 40 rows x [64] * 4 (edge rows):
2 x 1 tiles of 32x64, three seams - four times each on one stream and checks both outputs at every step: the on-device form of the
counter check. Every case leaves every switch at 0 and asynchronous mode as it found it. No case tries to starve a launch."""
import importlib
import os

import numpy as np
import pytest
import torch

from chain_edge_worker import BF16, GUARD_ROWS, orc
from chain_widths_worker import WidthsChain

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_dispatch.txt")
IMAGE_NAME = {2: "vnni2", 0: "flat", 4: "vnni4"}  # WidthsChain's image code -> the table's
STEPS = 6


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def switches(rt, v, width_rounds=None):
    rt.set_chain_edge(v), rt.set_chain_rounds(v), rt.set_chain_ragged(v), rt.set_chain_widths(v), rt.set_chain_widths_ragged(v), rt.set_chain_dma256(v)
    rt.set_chain_width_rounds(v if width_rounds is None or not v else width_rounds)
    rt.set_edge_tiles(2 * v), rt.set_edge_k_bf16(v), rt.set_edge_k8_bf16(v), rt.set_dma256_images(v)
    rt.force_variant(-1)


@pytest.fixture()
def sw(rt):
    """asynchronous mode for the case; whatever happens, every switch is 0 afterwards"""
    was_async = rt.set_async(True)
    switches(rt, 0)
    try:
        yield rt
    finally:
        rt.synchronize()
        switches(rt, 0)
        rt.set_async(was_async)


def counters(rt):
    return {"edge": rt.chain_edge_stats()[0], "rounds": rt.chain_rounds_stats()[0], "ragged": rt.chain_ragged_stats()[0], "widths": rt.chain_widths_stats()[0],
            "wrounds": rt.chain_width_rounds_stats()[0], "wragged": rt.chain_widths_ragged_stats()[0], "dma256": rt.chain_dma256_stats()[0]}


def golden_form(row, image):
    """the form of D(all) in the table's row for 256 compute units, strict off: 'plain', 'edge', .., or 'calls'"""
    for line in open(GOLDEN):
        cells = [c.strip() for c in line.split("|")]
        if len(cells) == 5 and cells[0] == row and cells[1] == "%s 256 0" % IMAGE_NAME[image]:
            return cells[4].split(":")[0]
    raise AssertionError("no row %r for image %s in %s" % (row, IMAGE_NAME[image], GOLDEN))


def layers(sizes, k_all=None):
    ns = sizes[1:]
    return ns, [k_all or k for k in sizes[:-1]]


def assert_exact(ch, ref):
    """the exactness precondition (chain_widths_worker.check_exact's, on oracle layers computed once): every layer of the oracle is the
    fp64 result of its own input, rounded once - so any order of additions gives these bits"""
    prev, v, rows = ch.x, ch.image or 1, ch.m + GUARD_ROWS
    for l in range(ch.L):
        K, n = ch.ks[l] * ch.brs[l], ch.ns[l]
        xin = orc.bf16_to_f32(prev).reshape(rows, -1)[:ch.m, :K].astype(np.float64)
        w = orc.bf16_to_f32(ch.W[l]).reshape(-1, ch.ldb[l], v)[:K // v, :n, :].transpose(0, 2, 1).reshape(K, n).astype(np.float64)
        f64 = np.maximum(xin @ w + orc.bf16_to_f32(ch.b[l])[:n].astype(np.float64)[None, :], 0)
        assert np.array_equal(orc.f32_to_bf16(f64.astype(np.float32).reshape(-1)).reshape(ch.m, n), ref[l].reshape(rows, ch.ldc[l])[:ch.m, :n]), "layer %d not exact" % l
        prev = ref[l]


def run_steps(rt, ch, ref, steps=STEPS):
    """`steps` chain invokes on refilled outputs, each compared with the oracle's layers and checked for writes outside the windows"""
    outs, ran = ch.outputs(), []
    for step in range(steps):
        if step:
            ch.refill(outs)
        ran.append(bool(rt.fused_brgemm_chain(BF16, ch.calls(outs))))
        got = ch.host(outs)
        ch.check_windows(got)
        for l in range(ch.L):
            bad = got[l] != ref[l]
            assert not bad.any(), "step %d layer %d: %d elements differ from the oracle, first at flat index %d" % (step, l, int(bad.sum()), int(np.argmax(bad)))
    return ran, got


# id, the golden table's row, rows, sizes, k of every layer (None: the input's width), images, forced width-rounds mode, the form if forced
CASES = [
    ("plain", "dev 64x[64]*3", 64, [64, 64, 64], None, (2, 0), None, None),
    ("edge_rows", "dev 100x[128]*3", 100, [128, 128, 128], None, (2, 4), None, None),
    ("ragged_width", "dev 200x[200]*4", 200, [200, 200, 200, 200], None, (2, 0), None, None),
    ("mixed_widths", "dev 256x[256,512,128,256]", 256, [256, 512, 128, 256], None, (2, 4), None, None),
    ("ragged_mixed_widths", "dev 200x[200,136,72,200]", 200, [200, 136, 72, 200], None, (2, 0), None, None),
    ("several_rounds", "dev 16448x[64]*3", 64 * 257, [64, 64, 64], None, (2, 4), None, None),
    # the regression case of tests/test_chain_dispatch.py: flat / VNNI-4 calls planned on 32x64 (257 tiles) ran in two rounds with both switches on
    ("edge_rows_in_front_of_rounds", "dev 8224x[64]*3", 32 * 257, [64, 64, 64], None, (0, 4), None, None),
    ("tile_256x256", "dev 7680x[64,2048,2048] k64", 7680, [64, 2048, 2048], 64, (2,), None, None),
    ("column_rounds_forced", "dev 256x[256,512,128,256]", 256, [256, 512, 128, 256], None, (2, 0), 1002, "wrounds"),
    ("refused_everywhere", "dev 64x[64,100,64]", 64, [64, 100, 64], None, (2, 4), None, None),
]


@pytest.mark.parametrize("name,row,m,sizes,k_all,images,width_rounds,forced_form", CASES, ids=[c[0] for c in CASES])
def test_every_switch_on_each_form_is_the_oracle_s_bits(sw, name, row, m, sizes, k_all, images, width_rounds, forced_form):
    rt = sw
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ns, ks = layers(sizes, k_all)
    for i, image in enumerate(images):
        ch = WidthsChain(rt, image, m, ns, ks, [1] * len(ns), 700 + 10 * len(name) + i, exact=True)
        ref = ch.oracle()
        assert_exact(ch, ref)
        switches(rt, 1, width_rounds)
        before = counters(rt)
        ran, got = run_steps(rt, ch, ref)
        after = counters(rt)
        want = forced_form or golden_form(row, image)
        moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
        print("%s %s: ran as one launch %s, counters moved %s, the table names %s" % (name, IMAGE_NAME[image], ran, moved, want))
        if cus == 256:
            assert ran == [want != "calls"] * STEPS, (ran, want)
            assert moved == ({} if want in ("calls", "plain") else {want: STEPS}), (moved, want)
        else:
            print("SKIPPED the counter check: the golden table is for 256 compute units, this device has %d" % cus)
            assert all(v == STEPS for v in moved.values()) and len(moved) <= 1, moved  # (still: one form, every step)
        # every switch at 0: the same bits (the chain contract, on exact data)
        switches(rt, 0)
        before = counters(rt)
        run_steps(rt, ch, ref, steps=1)
        assert counters(rt) == before, "a chain counter moved with every switch at 0"


def test_two_chains_that_share_a_counter_block_alternate_on_one_stream(sw):
    rt = sw
    a = WidthsChain(rt, 2, 64, [64, 64, 64], [64, 64, 64], [1, 1, 1], 811, exact=True)
    b = WidthsChain(rt, 2, 40, [64, 64, 64], [64, 64, 64], [1, 1, 1], 812, exact=True)
    ref_a, ref_b = a.oracle(), b.oracle()
    switches(rt, 1)
    before = counters(rt)
    outs_a, outs_b = a.outputs(), b.outputs()
    ran = []
    for step in range(4):
        for ch, outs, ref in ((a, outs_a, ref_a), (b, outs_b, ref_b)):
            ch.refill(outs)
            ran.append(bool(rt.fused_brgemm_chain(BF16, ch.calls(outs))))
            got = ch.host(outs)
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], ref[l]), "step %d, %d rows, layer %d differs from the oracle" % (step, ch.m, l)
    after = counters(rt)
    print("ran as one launch:", ran, "counters moved:", {k: after[k] - before[k] for k in after if after[k] != before[k]})
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert golden_form("dev 64x[64]*4", 2) == "plain" and golden_form("dev 40x[64]*4", 2) == "edge"
        assert all(ran) and {k: after[k] - before[k] for k in after if after[k] != before[k]} == {"edge": 4}
