"""Graph-captured replays of every launch form, bit for bit, on a real MI355X. `bench.py --graph` captures a step into a graph and reports
the faster of the two launch modes, and include/tpp_xsmm_abi.h / DESIGN.md promise one of three things about a captured stream for every
feature: the same kernel and the same bits (section 1), the unsplit launch (section 2, every launch that takes a block from
split_scratch_for), call by call (section 2, every chain form). The tile queue has rules of its own (section 3), and the scratch block
of the split kernels has edges no other test reaches (section 4).

Every capture is made the way tests/test_chain_gpu.py makes its one: a torch.cuda.Stream, xsmm_hip_set_stream, a warm-up outside the
capture, torch.cuda.graph(capture_error_mode="relaxed"), one stream and a linear graph (tests/graph_capture_worker.py captured). Inputs are
exact (tests/exact_data.py: every partial sum an integer an f32 holds), so the oracle's bits are the reference whatever kernel runs, after
the case's own precondition - the oracle equals the fp64 result rounded once. Each graph is replayed three times; before each replay the
inputs are overwritten in place with fresh exact data and the outputs refilled with NaN; after it the output window equals the oracle's
bits for that input and the whole output buffer equals the same call made un-captured - guard rows, gap columns and the bit pattern
around the window included. There is no tolerance anywhere in this file. What a call reports - the kernel text, the counters - is
asserted for the call inside the capture as for the call outside it. Every switch is 0 (xsmm_hip_set_f32_halves: as found) afterwards.

  1 forms that are legal in a capture, one smallest eligible shape per form under its forcing mode (the shapes of the form's own test
    file): f32 edge tile, f32 ragged k, f32 halves, bf16 edge tile, bf16 ragged k, bf16 k8, the 256x256 flat and VNNI-4 images, the
    256x256 edge tiles, the skinny bf16 kernel on every (image, BN) instance at m = 17, n = BN + 8, k = 72 (clamped rows, a shifted block
    and a ragged tail inside the graph). Inside the capture the call reports the same kernel and moves the same counter as outside it,
    and no other counter moves - single-call, chain or tile-queue.
  2 forms that fall back in a capture. Splits - a forced split count on the f32 loader-wave variants, the tail split at the smallest
    shape the CU count gives, skinny split P = 3 at k = 72 and P = 16 at (k, br) = (64, 16): inside the capture the reported kernel is the
    unsplit one, the split's counter stands still and the unsplit counter moves where there is one; between the replays the same call
    runs un-captured on the same stream and IS the split kernel. (The split of brgemm_bf16_small.hip lives in tile-queue groups: in the
    worker, with section 3.) Chains - every case of tests/test_chain_switches_gpu.py CASES with all switches on, and a skinny chain
    (m = 17, [3 BN + 8] * 3, k0 = 72): inside a capture xsmm_hip_fused_brgemm_chain_invoke returns 0 and no chain counter moves; every
    replay equals the oracle layer by layer and the un-captured chain invoke under the same switches. (On exact inputs every form has
    the oracle's bits, so that comparison holds for every form - also where, on random data, the two tile families differ by an ulp as
    tests/test_chain_gpu.py notes: there the comparison would have to be with the call-by-call run.) The largest case (7680 rows x 2048
    columns) draws one fresh input; its second and third are row permutations of it, checked against the same permutation of its oracle rows.
  3 the tile queue in a capture, 4 the scratch block's edges: tests/graph_capture_worker.py, a process per scenario (the slot ring, the
    trace cache and the scratch blocks are per process and never freed; a library that exits is a failed assertion here, not a dead pytest)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_data as ed
from chain_edge_worker import GUARD_ROWS, NAN
from chain_widths_worker import WidthsChain
from graph_capture_worker import BF16, F32, SLOTS, Case, F32Case, captured, download, invoke, same_bits, upload
from skinny_bf16_worker import expected_stats as skinny_stats
from skinny_bf16_worker import instance_exists
from skinny_bf16_worker import text as skinny_text
from skinny_split_worker import expected_skinny_stats, expected_split_stats
from skinny_split_worker import text as split_text
from test_tail_split_gpu import shape as tail_shape
from test_chain_switches_gpu import CASES as CHAIN_CASES
from test_chain_switches_gpu import assert_exact, golden_form, layers
from test_chain_switches_gpu import counters as chain_counters
from test_chain_switches_gpu import switches as chain_switches

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_NAME = {6: "brgemm_f32_lw<64x64,k2>", 7: "brgemm_f32_lw<64x32,k4>", 9: "brgemm_f32_lw<32x32,k4>"}
F32_TILE = {6: (64, 64), 7: (64, 32), 9: (32, 32)}
DMA_KIND = {2: 0, 0: 2, 4: 4}
EP = dict(beta0=True, bias=True, relu=True)  # beta 0: the output window is NaN before every run
SINGLE = ("edge_tiles", "edge_k", "edge_k_bf16", "edge_k8_bf16", "dma256_images", "dma256_edge", "skinny_bf16", "skinny_split", "tail_split", "f32_halves")


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def all_off(rt):
    for name in SINGLE:
        if name != "f32_halves":
            getattr(rt, "set_" + name)(0)
    chain_switches(rt, 0)
    rt.set_chain_skinny(0)
    rt.force_split(-1)
    rt.force_variant(-1)
    rt.set_stream(None)


@pytest.fixture(autouse=True)
def sw(rt):
    """asynchronous mode for the case (nothing may synchronise inside a capture); whatever happens, every switch is 0 afterwards"""
    was_async, halves = rt.set_async(True), rt.set_f32_halves(0)
    rt.set_f32_halves(halves)
    all_off(rt)
    try:
        yield rt
    finally:
        all_off(rt)
        rt.set_f32_halves(halves)
        rt.synchronize()
        torch.cuda.synchronize()
        rt.set_async(was_async)


def counters(rt):
    c = {name: getattr(rt, name + "_stats")() for name in SINGLE}
    c["chains"], c["tile_queue"] = all_chain_counters(rt), rt.tile_queue_stats()
    return c


def all_chain_counters(rt):
    c = chain_counters(rt)
    c["skinny"] = rt.chain_skinny_stats()[0]
    return c


def observed(rt, case, h, bufs):
    """the call, with what it reported and where every single-call counter stood before and after it"""
    before = counters(rt)
    refined = invoke(rt, case, h, bufs)
    return refined, before, counters(rt)


def assert_report(obs, text, moved, where):
    """the reported kernel is `text`; exactly the counters of `moved` (name -> the tuple behind the launch count) went up by one launch
    and describe this launch; every other single-call counter stands still"""
    refined, before, after = obs
    assert refined == text, (where, refined, text)
    for name in SINGLE:
        if name in moved:
            assert after[name] == (before[name][0] + 1,) + tuple(moved[name]), (where, name, before[name], after[name])
        else:
            assert after[name] == before[name], (where, name, before[name], after[name])
    for name in ("chains", "tile_queue"):  # a whole-layer call is no chain launch and never passes through the tile queue
        assert after[name] == before[name], (where, name, before[name], after[name])


def assert_exact_case(case):
    ref = case.oracle()
    assert np.array_equal(ed.bits(ref[case.win]), ed.bits(case.fp64())), "not an exact case: the oracle is not the fp64 result rounded once"
    assert case.outside_untouched(ref)
    return ref


def replay_three_times(rt, graph, make, h, bufs_g, bufs_r, seed, between=None, what=""):
    """three replays of `graph` (the call on bufs_g) on fresh exact inputs and NaN-refilled outputs: the oracle's bits, the bits of the same
    call un-captured (on bufs_r) over the whole C buffer, nothing outside the window written, the operands as uploaded. between(fresh):
    the un-captured call of the case - returns what `observed` returns - made after the replay"""
    for rep in range(3):
        fresh = make(seed + 1 + rep)
        ref = assert_exact_case(fresh)
        upload(bufs_g, fresh)
        upload(bufs_r, fresh)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got_g = download(bufs_g[2], fresh)
        obs = between(fresh) if between else observed(rt, fresh, h, bufs_r)
        rt.synchronize()
        torch.cuda.synchronize()
        got_r = download(bufs_r[2], fresh)
        ed.check_bits(got_g[fresh.win], ref[fresh.win], F32 if fresh.image is None else BF16, "%s, replay %d" % (what, rep))
        assert fresh.outside_untouched(got_g), "%s, replay %d: wrote outside the m x n window" % (what, rep)
        assert same_bits(got_g, got_r), "%s, replay %d: differs from the same call made un-captured" % (what, rep)
        for d, host in zip((bufs_g[0], bufs_g[1], bufs_g[3]), (fresh.A, fresh.B, fresh.D)):
            assert same_bits(download(d, fresh), host), "%s, replay %d: an input operand was written" % (what, rep)
        yield rep, obs


# ------------------------------------------------------------------------------------------------ 1: legal in a capture
def f32_form(name, m, n, k, br, on, text, moved, force=None):
    return dict(id=name, make=lambda seed: F32Case(m, n, k, br, seed, **EP), on=on, text=text, moved=moved, force=force)


def bf16_form(name, image, m, n, k, br, on, text, moved):
    return dict(id=name, make=lambda seed: Case(image, m, n, k, br, seed, exact=True, **EP), on=on, text=text, moved=moved, force=None)


FORMS = [
    # tests/test_edge_tiles_gpu.py shapes(9)[0]: one more row than the 32x32 tile, one more 16-byte piece of columns
    f32_form("f32_edge_tile", 33, 36, 64, 1, [("edge_tiles", 9)], F32_NAME[9] + ", edge tiles", {"edge_tiles": (2, 2, 9)}),
    # tests/test_edge_k_gpu.py: 2 x 2 tiles of variant 9, the smallest k of KS
    f32_form("f32_ragged_k", 64, 64, 72, 1, [("edge_k", 9)], F32_NAME[9] + ", ragged k", {"edge_k": (2, 56, 9)}),
    # tests/test_f32_halves_gpu.py CASES[0]: one 64x64 + K2 tile, two halves (the form keeps the kernel name and reports no text)
    f32_form("f32_halves", 64, 64, 64, 1, [("f32_halves", 2)], "", {"f32_halves": (1, 1, 0)}, force=6),
    # tests/test_edge_tiles_bf16_gpu.py shapes(0)[0] on the 32x64 + K2 tile
    bf16_form("bf16_edge_tile", 2, 33, 72, 64, 1, [("edge_tiles", 20)], "brgemm_bf16_lw<32x64,k2>, edge tiles", {"edge_tiles": (2, 2, 20)}),
    # tests/test_edge_k_bf16_gpu.py / test_edge_k8_bf16_gpu.py: 2 x 2 tiles of tile 0, the smallest k of KS
    bf16_form("bf16_ragged_k", 2, 64, 128, 80, 1, [("edge_k_bf16", 20)], "brgemm_bf16_lw<32x64,k2>, ragged k", {"edge_k_bf16": (2, 48, 20)}),
    bf16_form("bf16_k8", 2, 64, 128, 72, 1, [("edge_k8_bf16", 20)], "brgemm_bf16_lw<32x64,k2>, ragged k, half step", {"edge_k8_bf16": (2, 56, 20)}),
    # tests/test_dma256_images_gpu.py SHAPES[0], KBR[0]; tests/test_dma256_edge_gpu.py SHAPES[0], KBR[0]
    bf16_form("dma256_flat", 0, 256, 256, 64, 1, [("dma256_images", 2)], "brgemm_bf16_dma_flatb<256x256>", {"dma256_images": (1, 1, 2)}),
    bf16_form("dma256_vnni4", 4, 256, 256, 64, 1, [("dma256_images", 2)], "brgemm_bf16_dma_vnni4<256x256>", {"dma256_images": (1, 1, 4)}),
    bf16_form("dma256_edge", 2, 264, 256, 32, 1, [("dma256_edge", 2)], "brgemm_bf16_dma<256x256>, edge tiles", {"dma256_edge": (2, 1, DMA_KIND[2])}),
] + [
    bf16_form("skinny_%d_bn%d" % (image, bn), image, 17, bn + 8, 72, 1, [("skinny_bf16", bn)], skinny_text(image, 17, bn),
              {"skinny_bf16": skinny_stats(0, image, bn + 8, 72, 1, bn)[1:]})
    for image in (2, 0, 4) for bn in (16, 32, 64) if instance_exists(image, bn)
]


@pytest.mark.parametrize("form", FORMS, ids=[f["id"] for f in FORMS])
def test_a_form_that_is_legal_in_a_capture_is_the_same_kernel_and_the_same_bits(rt, form):
    seed = 100 + 7 * FORMS.index(form)
    case = form["make"](seed)
    assert_exact_case(case)
    h = case.dispatch(rt, form["force"])
    if form["id"] == "f32_halves":
        assert "64x64,k2" in rt.kernel_name(h), rt.kernel_name(h)
    bufs_g, bufs_r = case.device(), case.device()
    for name, value in form["on"]:
        assert getattr(rt, "set_" + name)(value) >= 0
    graph, inside, _ = captured(rt, lambda: observed(rt, case, h, bufs_g))
    assert_report(inside, form["text"], form["moved"], "inside the capture")
    assert_report(observed(rt, case, h, bufs_r), form["text"], form["moved"], "outside the capture")
    for rep, obs in replay_three_times(rt, graph, form["make"], h, bufs_g, bufs_r, seed, what=form["id"]):
        assert_report(obs, form["text"], form["moved"], "un-captured, after replay %d" % rep)


# ------------------------------------------------------------------------------------------------ 2: falls back in a capture - splits
def run_split(rt, make, seed, force, on, split_text_, split_moved, unsplit_text, unsplit_moved, what):
    """the call with its split forced on: captured it is the unsplit launch; un-captured on the capture's stream it is the split one"""
    case = make(seed)
    assert_exact_case(case)
    h = case.dispatch(rt, force)
    bufs_g, bufs_r = case.device(), case.device()
    on(rt)
    graph, inside, s = captured(rt, lambda: observed(rt, case, h, bufs_g))
    assert_report(inside, unsplit_text, unsplit_moved, what + ", inside the capture")

    def split_on_the_same_stream(fresh):
        try:
            rt.set_stream(s)
            return observed(rt, fresh, h, bufs_r)
        finally:
            rt.set_stream(None)

    assert_report(split_on_the_same_stream(case), split_text_, split_moved, what + ", un-captured on the capture's stream")
    for rep, obs in replay_three_times(rt, graph, make, h, bufs_g, bufs_r, seed, between=split_on_the_same_stream, what=what):
        assert_report(obs, split_text_, split_moved, what + ", un-captured after replay %d" % rep)


# tests/test_exact_gpu.py SPLIT_CASES: the smallest shape per loader-wave variant that splits under a forced count
F32_SPLITS = [(6, 128, 256, 64, 7), (7, 64, 96, 64, 5), (9, 96, 160, 128, 3)]


@pytest.mark.parametrize("variant,m,n,k,br", F32_SPLITS, ids=["v%d" % c[0] for c in F32_SPLITS])
def test_a_forced_f32_split_runs_unsplit_in_a_capture(rt, variant, m, n, k, br):
    run_split(rt, lambda seed: F32Case(m, n, k, br, seed, **EP), 40 + variant, variant, lambda r: r.force_split(2),
              F32_NAME[variant] + ", split", {}, "", {}, "forced split of variant %d" % variant)


def test_the_tail_split_runs_unsplit_in_a_capture(rt):
    """tests/test_tail_split_gpu.py shape(9, 16) under setting 2: 16 tile rows of the 32x32 tile, one round of tiles and 16 tail tiles"""
    m, n, r, cus = tail_shape(9, 16)
    run_split(rt, lambda seed: F32Case(m, n, 64, 4, seed, **EP), 60, 9, lambda r_: r_.set_tail_split(2),
              F32_NAME[9] + ", tail split", {"tail_split": (r, 2, cus)}, "", {}, "tail split")


@pytest.mark.parametrize("P,k,br", [(3, 72, 1), (16, 64, 16)], ids=["P3_k72", "P16_k64_br16"])
def test_the_skinny_split_runs_unsplit_in_a_capture(rt, P, k, br):
    image, bn, m, n = 2, 32, 17, 32 + 8

    def on(r):
        r.set_skinny_bf16(bn), r.set_skinny_split(P)

    run_split(rt, lambda seed: Case(image, m, n, k, br, seed, exact=True, **EP), 80 + P, None, on,
              split_text(image, m, bn), {"skinny_split": expected_split_stats(0, n, k, br, bn, P)[1:], "skinny_bf16": expected_skinny_stats(0, image, n, k, br, bn, P)[1:]},
              skinny_text(image, m, bn), {"skinny_bf16": skinny_stats(0, image, n, k, br, bn)[1:]}, "skinny split P = %d" % P)


# ------------------------------------------------------------------------------------------------ 2: falls back in a capture - chains
ALL_CHAIN_CASES = [c + (None,) for c in CHAIN_CASES] + [("skinny_chain", None, 17, [72] + [3 * 32 + 8] * 3, None, (2,), None, None, 32)]


@pytest.mark.parametrize("name,row,m,sizes,k_all,images,width_rounds,forced_form,skinny", ALL_CHAIN_CASES, ids=[c[0] for c in ALL_CHAIN_CASES])
def test_a_captured_chain_runs_call_by_call(rt, name, row, m, sizes, k_all, images, width_rounds, forced_form, skinny):
    ns, ks = layers(sizes, k_all)
    for i, image in enumerate(images):
        ch = WidthsChain(rt, image, m, ns, ks, [1] * len(ns), 900 + 10 * len(name) + i, exact=True)
        outs_g, outs_r = ch.outputs(), ch.outputs()
        if skinny:
            rt.set_chain_skinny(skinny)
        else:
            chain_switches(rt, 1, width_rounds)

        log = []  # every call: (ran as one launch, the chain counters before, after)

        def call(outs=outs_g):
            before = all_chain_counters(rt)
            log.append((bool(rt.fused_brgemm_chain(BF16, ch.calls(outs))), before, all_chain_counters(rt)))
            return log[-1]

        def assert_one_launch_where_the_form_has_one(obs, where):
            """the un-captured call: the return value and the one counter that moved are the form's, as tests/test_chain_switches_gpu.py
            asserts them - D(all) of the golden table's row (256 compute units: the table's), the skinny counter for the skinny chain"""
            fused, before, after = obs
            moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
            if skinny:
                assert fused is True and moved == {"skinny": 1}, (where, name, fused, moved)
            elif torch.cuda.get_device_properties(0).multi_processor_count == 256:
                want = forced_form or golden_form(row, image)
                assert fused is (want != "calls"), (where, name, image, fused, want)
                assert moved == ({} if want in ("calls", "plain") else {want: 1}), (where, name, image, moved, want)
            else:
                assert len(moved) <= 1 and all(v == 1 for v in moved.values()), (where, name, image, moved)

        graph, (fused, before, after), _ = captured(rt, call)
        assert fused is False, "%s image %d: a captured chain call must not use a one-launch kernel" % (name, image)
        assert after == before, ("a chain counter moved inside the capture", name, before, after)
        assert len(log) == 2
        assert_one_launch_where_the_form_has_one(log[0], "the warm-up in front of the capture")
        rows, rng = m + GUARD_ROWS, np.random.default_rng(5 + i)
        # The oracle costs seconds on the largest case (7680 x 2048 per layer). The rows of a chain are independent - row r of every layer
        # is a function of row r of the input alone - so there the second and third input are row permutations of the first, new draw,
        # and their reference is the same permutation of ITS oracle rows: the oracle's bits for that input, computed once.
        shuffle_rows = m * max(ns) > 1 << 22
        for rep in range(3):
            x = np.full((rows, ch.ld_in[0]), NAN, np.uint16)  # fresh exact input, the NaN guard rows and gap columns as WidthsChain lays them
            if rep == 0 or not shuffle_rows:
                x[:m, :ks[0]] = ed.store(rng.integers(-15, 16, (m, ks[0])), BF16).reshape(m, ks[0])
                ch.x = x.reshape(-1)
                ref = ch.oracle()
                assert_exact(ch, ref)
            else:
                perm = rng.permutation(m)
                x[:m] = ch.x.reshape(rows, -1)[:m][perm]
                ch.x = x.reshape(-1)
                for l in range(ch.L):
                    r2 = ref[l].reshape(rows, ch.ldc[l]).copy()
                    r2[:m] = r2[:m][perm]
                    ref[l] = r2.reshape(-1)
            ch.dx.copy_(torch.from_numpy(ch.x.view(np.int16)).cuda())
            ch.refill(outs_g)
            ch.refill(outs_r)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            got = ch.host(outs_g)
            ch.check_windows(got)
            for l in range(ch.L):
                assert np.array_equal(got[l], ref[l]), "%s image %d, replay %d: layer %d differs from the oracle" % (name, image, rep, l)
            assert_one_launch_where_the_form_has_one(call(outs_r), "un-captured, after replay %d" % rep)  # under the same switches
            rt.synchronize()
            for l in range(ch.L):  # (whole buffers, compared on the device: the largest case has 31 MB per layer)
                assert torch.equal(outs_g[l], outs_r[l]), "%s image %d, replay %d: layer %d differs from the un-captured chain invoke" % (name, image, rep, l)
        chain_switches(rt, 0)
        rt.set_chain_skinny(0)


# ------------------------------------------------------------------------------------------------ 3, 4: in a process of their own
def worker(*args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "graph_capture_worker.py")] + list(args), capture_output=True, text=True, env=env, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, "the worker ended with status %d and no result: %s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
    d = json.loads(lines[-1])
    print(json.dumps({k: v for k, v in d.items() if k != "errors"}))
    assert d["errors"] == [], d["errors"][:8]
    return d


@pytest.mark.parametrize("scenario", ["cold", "warm"])
def test_a_captured_tile_queue_group_keeps_its_work_list(scenario):
    """cold: the captured flush gathers into a pinned slot of the ring; warm: the whole group replays from its segment's device list, and a
    second group in the same capture takes the pinned slot. The captured slot-taking flush is the eighth of its slot group. More than 40
    un-captured flushes before every replay: every ring slot and every event group is used again, the segment is evicted"""
    d = worker("queue", scenario)
    assert d["replays"] == [True, True, True]
    assert d["in_capture"][0] == (2 if scenario == "warm" else 1), d["in_capture"]  # grouped launches inside the capture
    assert d["flushes"] >= 3 * 40 and d["slot_flushes"] >= 3 * SLOTS and d["recorded_groups"] > 64, d


def test_a_captured_bf16_small_group_runs_unsplit():
    d = worker("small")
    assert d["replays"] == [True, True, True]
    assert d["outside"] == ["brgemm_bf16_small32 grouped, split"] * 3, d["outside"]
    assert d["inside"] == "brgemm_bf16_small32 grouped", d["inside"]


def test_the_scratch_block_grows_under_launches_in_flight():
    d = worker("growth")
    assert d["split_launches"] == 3 and len(d["kernels"]) == 3


def test_the_seventeenth_stream_runs_unsplit():
    d = worker("streams")
    assert d["split_moved"] == [1] * 16 + [0, 0] and d["skinny_moved"] == [1] * 18, d
