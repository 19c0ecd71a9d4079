"""The K split inside a skinny-batch f32 chain launch (include/tpp_xsmm_abi.h xsmm_hip_set_chain_skinny_f32_split) on a real MI355X: under
xsmm_hip_set_chain_skinny_f32(BN) + xsmm_hip_set_chain_skinny_f32_split(P) an f32 chain with 1 <= m <= 31 rows runs as ONE launch of
brgemm_f32_skinny_chain_split<BN, MB> with the bits of the same calls one by one under xsmm_hip_set_skinny_f32(BN) + xsmm_hip_set_skinny_f32_split(P).
The two chains are test_chain_skinny_f32_split_cpu.chains (the CPU walk takes the same); buffers, guards and the fp64 check are those of
tests/test_chain_skinny_f32_gpu.py. Every case leaves every switch 0. Nothing tries to starve a launch."""
import numpy as np
import pytest
import torch

from chain_edge_worker import F32, GUARD_ROWS, dev
from chain_widths_worker import WidthsChain
from test_chain_skinny_f32_gpu import all_off, check_exact, cus, one_by_one, others, rt, run_chain, same_bits  # noqa: F401 (rt: the fixture)
from test_chain_skinny_f32_split_cpu import chains, schedule

pytestmark = pytest.mark.gpu
BNS = [16, 32, 64]


@pytest.fixture()
def sw(rt):  # noqa: F811
    """asynchronous mode for the case; whatever happens, every switch is 0 afterwards"""
    was_async = rt.set_async(True)
    all_off(rt), rt.set_chain_skinny_f32_split(0)
    try:
        yield rt
    finally:
        rt.synchronize()
        all_off(rt), rt.set_chain_skinny_f32_split(0)
        rt.set_async(was_async)


def run_split(rt, ch, bn, P, G=None, outs=None):
    """the chain under BN `bn` (on G workgroups if forced) and P parts: one launch, the split counter moved by one and holds (P, G), the chain
    counter by one and holds (G, BN, the waves of the deepest part), no other counter moved"""
    _, units, waves, _, _ = schedule(bn, 16 if ch.m <= 16 else 32, P, ch.ns, ch.ks, ch.brs)
    rt.set_chain_skinny_f32(bn if G is None else 1000 * G + bn)
    rt.set_chain_skinny_f32_split(P)
    G = min(units, cus()) if G is None else G
    before, cbefore, o = rt.chain_skinny_f32_split_stats(), rt.chain_skinny_f32_stats(), others(rt)
    ran, got = run_chain(rt, ch, outs)
    rt.set_chain_skinny_f32_split(0), rt.set_chain_skinny_f32(0)
    assert ran, "the chain ran call by call"
    assert rt.chain_skinny_f32_split_stats() == (before[0] + 1, P, G), (before, rt.chain_skinny_f32_split_stats())
    assert rt.chain_skinny_f32_stats() == (cbefore[0] + 1, G, bn, waves), (cbefore, rt.chain_skinny_f32_stats())
    assert others(rt) == o, "another counter moved"
    return got


def split_one_by_one(rt, ch, bn, P, outs):
    """the same calls one by one on the split skinny f32 kernel: every layer with two steps or more moves its counter"""
    rt.set_skinny_f32_split(P)
    before = rt.skinny_f32_split_stats()[0]
    got = one_by_one(rt, ch, bn, outs)
    rt.set_skinny_f32_split(0)
    assert rt.skinny_f32_split_stats()[0] == before + sum(br * -(-k // 16) >= 2 for k, br in zip(ch.ks, ch.brs)), "a reference call did not run split"
    return got


@pytest.mark.parametrize("G", [None, 1, 3], ids=["rule", "G1", "G3"])
@pytest.mark.parametrize("P", [2, 3, 16])
@pytest.mark.parametrize("bn", BNS)
def test_exact_inputs_every_layer_bit_for_bit_fp64(sw, bn, P, G):
    """G 1: one workgroup is the last arriver of every block; G 3 with P 2: a workgroup walks several units, parts of different blocks"""
    for name, ns, ks, brs in chains(bn):
        for m in (1, 16, 17, 31):
            ch = WidthsChain(sw, 0, m, ns, ks, brs, 31 * m + bn + P + len(name), exact=True, dtype=F32)
            check_exact(ch, run_split(sw, ch, bn, P, G))


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("bn", BNS)
def test_steps_back_to_back_equal_the_split_calls_one_by_one(sw, bn, P):
    """random inputs, four steps with other layer-0 inputs and no synchronisation in between, three times over: the arrival counters' reset,
    the epochs, the one scratch region under every layer and launch"""
    rt, steps = sw, 4
    rt.set_stream(torch.cuda.current_stream())  # (the stream torch's copies below are queued on)
    for name, ns, ks, brs in chains(bn):
        for m in (1, 31):
            ch = WidthsChain(rt, 0, m, ns, ks, brs, 77 + 31 * m + bn + P, dtype=F32)
            rng, k, x0, xs = np.random.default_rng(m + bn + P), ks[0] * brs[0], ch.dx, []
            for _ in range(steps):
                X = ch.x.copy().reshape(m + GUARD_ROWS, ch.ld_in[0])
                X[:m, :k] = rng.uniform(-1, 1, (m, k)).astype(np.float32)
                xs.append(dev(X.reshape(-1)))
            outs, want = ch.outputs(), []
            for x in xs:
                ch.dx = x
                want.append(split_one_by_one(rt, ch, bn, P, outs))
            ch.dx = x0
            run_split(rt, ch, bn, P)  # (the block's first launch is followed by a synchronisation: not in the loop below)
            for rep in range(3):
                ch.refill(outs)
                rt.set_chain_skinny_f32(bn), rt.set_chain_skinny_f32_split(P)
                before, stash, ran = rt.chain_skinny_f32_split_stats()[0], [], []
                for x in xs:  # no synchronisation in here: the copies are stream-ordered behind each launch
                    ch.dx = x
                    ran.append(rt.fused_brgemm_chain(F32, ch.calls(outs)))
                    stash.append([o.clone() for o in outs])
                rt.set_chain_skinny_f32_split(0), rt.set_chain_skinny_f32(0)
                ch.dx = x0
                rt.synchronize()
                torch.cuda.synchronize()
                assert all(ran) and rt.chain_skinny_f32_split_stats()[0] == before + steps, ran
                for step, s in enumerate(stash):
                    got = [o.cpu().numpy() for o in s]
                    ch.check_windows(got)
                    same_bits(got, want[step], "%s m %d repeat %d step %d" % (name, m, rep, step))


def test_the_switch_alone_changes_nothing(sw):
    rt = sw
    name, ns, ks, brs = chains(32)[0]
    ch = WidthsChain(rt, 0, 16, ns, ks, brs, 5, dtype=F32)
    before = rt.chain_skinny_f32_split_stats(), rt.chain_skinny_f32_stats()
    rt.set_chain_skinny_f32_split(4)
    ran_on, got = run_chain(rt, ch)
    rt.set_chain_skinny_f32_split(0)
    ran_off, want = run_chain(rt, ch)
    assert ran_on == ran_off and (rt.chain_skinny_f32_split_stats(), rt.chain_skinny_f32_stats()) == before
    same_bits(got, want, "chain_skinny_f32 at 0")


def test_a_stream_without_a_scratch_block_runs_the_unsplit_launch(sw):
    """the kernel file keeps its own list of 16 scratch blocks (split_scratch.h): with the default stream's and 16 fresh streams the last one has
    none - its launch is the unsplit chain's on the same G, with that form's bits and the split counter still. (Last in the file: the list
    is full from here on.)"""
    rt, bn, P = sw, 32, 2
    name, ns, ks, brs = chains(bn)[0]
    ch = WidthsChain(rt, 0, 17, ns, ks, brs, 23, dtype=F32)
    _, units, _, _, _ = schedule(bn, 32, P, ns, ks, brs)
    want_unsplit, want_split = one_by_one(rt, ch, bn), split_one_by_one(rt, ch, bn, P, ch.outputs())
    assert not all(np.array_equal(a, b) for a, b in zip(want_unsplit, want_split)), "the two forms must differ in some bit for this test to see anything"
    same_bits(run_split(rt, ch, bn, P), want_split, "the default stream")
    torch.cuda.synchronize()
    moved = []
    for s in [torch.cuda.Stream() for _ in range(16)]:
        outs = ch.outputs()
        torch.cuda.synchronize()
        before, cbefore = rt.chain_skinny_f32_split_stats()[0], rt.chain_skinny_f32_stats()[0]
        rt.set_chain_skinny_f32(bn), rt.set_chain_skinny_f32_split(P)
        try:
            rt.set_stream(s)
            ran = rt.fused_brgemm_chain(F32, ch.calls(outs))
            rt.synchronize()
        finally:
            rt.set_stream(None)
            rt.set_chain_skinny_f32_split(0), rt.set_chain_skinny_f32(0)
        s.synchronize()
        got = ch.host(outs)
        ch.check_windows(got)
        moved.append(rt.chain_skinny_f32_split_stats()[0] - before)
        assert ran and rt.chain_skinny_f32_stats()[:3] == (cbefore + 1, min(units, cus()), bn), "one launch of the chain form on the split's G"
        same_bits(got, want_split if moved[-1] else want_unsplit, "stream %d" % len(moved))
    assert moved[0] == 1 and moved[-1] == 0 and moved == sorted(moved, reverse=True), moved
