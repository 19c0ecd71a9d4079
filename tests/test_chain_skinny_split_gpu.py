"""The K split inside a skinny-batch bf16 chain launch (include/tpp_xsmm_abi.h xsmm_hip_set_chain_skinny_split) on a real MI355X: under
xsmm_hip_set_chain_skinny(BN) + xsmm_hip_set_chain_skinny_split(P) a bf16 chain with 1 <= m <= 31 rows runs as ONE launch of
brgemm_bf16_skinny_chain_split<IMG, BN, MB> with the bits of the same calls one by one under xsmm_hip_set_skinny_bf16(BN) + xsmm_hip_set_skinny_split(P).
The chains are test_chain_skinny_gpu.chains (k from 32 to 264: one to nine steps - a ragged last step, a one-step layer inside a split launch,
workgroups that sit a layer out, batches, eight layers); buffers, guards and the fp64 check are that file's. Every case leaves every switch
0. Nothing tries to starve a launch."""
import numpy as np
import pytest
import torch

from chain_edge_worker import BF16, GUARD_ROWS, dev, orc
from chain_skinny_worker import KIND, run_chain
from chain_widths_worker import WidthsChain, check_exact
from test_chain_skinny_gpu import INSTANCES, all_off, chains, cus, one_by_one, others, rt, variants  # noqa: F401 (rt: the fixture)
from test_chain_skinny_split_cpu import schedule

pytestmark = pytest.mark.gpu


@pytest.fixture()
def sw(rt):  # noqa: F811
    """asynchronous mode for the case; whatever happens, every switch is 0 afterwards"""
    was_async = rt.set_async(True)
    all_off(rt), rt.set_chain_skinny_split(0)
    try:
        yield rt
    finally:
        rt.synchronize()
        all_off(rt), rt.set_chain_skinny_split(0)
        rt.set_async(was_async)


def same_bits(got, want, what):
    for l, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), "%s: layer %d differs" % (what, l)


def run_split(rt, ch, bn, P, G=None, outs=None):
    """the chain under BN `bn` (on G workgroups if forced) and P parts: one launch, the split counter moved by one and holds (P, G), the chain
    counter by one and holds (G, BN, image), no other counter moved"""
    _, units, _, _, _ = schedule(bn, 16 if ch.m <= 16 else 32, P, ch.ns, ch.ks, ch.brs)
    rt.set_chain_skinny(bn if G is None else 1000 * G + bn)
    rt.set_chain_skinny_split(P)
    G = min(units, cus()) if G is None else G
    before, cbefore, o = rt.chain_skinny_split_stats(), rt.chain_skinny_stats(), others(rt)
    ran, got = run_chain(rt, ch, outs)
    rt.set_chain_skinny_split(0), rt.set_chain_skinny(0)
    assert ran, "the chain ran call by call"
    assert rt.chain_skinny_split_stats() == (before[0] + 1, P, G), (before, rt.chain_skinny_split_stats())
    assert rt.chain_skinny_stats() == (cbefore[0] + 1, G, bn, KIND[ch.image]), (cbefore, rt.chain_skinny_stats())
    assert others(rt) == o, "another counter moved"
    return got


def split_one_by_one(rt, ch, bn, P, outs=None, windows=True):
    """the same calls one by one on the split skinny kernel: every layer with two steps or more moves its counter"""
    rt.set_skinny_split(P)
    before = rt.skinny_split_stats()[0]
    got = one_by_one(rt, ch, bn, outs, windows)
    rt.set_skinny_split(0)
    assert rt.skinny_split_stats()[0] == before + sum(br * -(-k // 32) >= 2 for k, br in zip(ch.ks, ch.brs)), "a reference call did not run split"
    return got


@pytest.mark.parametrize("G", [None, 1, 3], ids=["rule", "G1", "G3"])
@pytest.mark.parametrize("P", [2, 3, 16])
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_exact_inputs_every_layer_bit_for_bit_fp64(sw, image, bn, P, G):
    """G 1: one workgroup is the last arriver of every block; G 3 with P 2: a workgroup walks several units, parts of different blocks"""
    for name, ns, ks, brs in chains(bn):
        for m in (1, 16, 17, 31):
            ch = WidthsChain(sw, image, m, ns, ks, brs, 1000 * image + 31 * m + bn + P + len(name), exact=True)
            check_exact(ch, run_split(sw, ch, bn, P, G))


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_steps_back_to_back_equal_the_split_calls_one_by_one(sw, image, bn, P):
    """random inputs, four steps with other layer-0 inputs and no synchronisation in between, three times over: the arrival counters' reset,
    the epochs, the one scratch region under every layer and launch"""
    rt, steps = sw, 4
    rt.set_stream(torch.cuda.current_stream())  # (the stream torch's copies below are queued on)
    for name, ns, ks, brs in chains(bn):
        for m in (1, 31):
            ch = WidthsChain(rt, image, m, ns, ks, brs, 77 * image + 31 * m + bn + P + len(name))
            xs, x0 = variants(ch, steps, m + bn + P), ch.dx
            outs, want = ch.outputs(), []
            for x in xs:
                ch.dx = x
                want.append(split_one_by_one(rt, ch, bn, P, outs, windows=False))
            ch.dx = x0
            run_split(rt, ch, bn, P)  # (the block's first launch is followed by a synchronisation: not in the loop below)
            for rep in range(3):
                ch.refill(outs)
                rt.set_chain_skinny(bn), rt.set_chain_skinny_split(P)
                before, stash, ran = rt.chain_skinny_split_stats()[0], [], []
                for x in xs:  # no synchronisation in here: the copies are stream-ordered behind each launch
                    ch.dx = x
                    ran.append(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
                    stash.append([o.clone() for o in outs])
                rt.set_chain_skinny_split(0), rt.set_chain_skinny(0)
                ch.dx = x0
                rt.synchronize()
                torch.cuda.synchronize()
                assert all(ran) and rt.chain_skinny_split_stats()[0] == before + steps, ran
                for step, s in enumerate(stash):
                    got = [o.cpu().numpy().view(np.uint16) for o in s]
                    ch.check_windows(got)
                    same_bits(got, want[step], "%s m %d repeat %d step %d" % (name, m, rep, step))


def test_the_switch_alone_changes_nothing(sw):
    rt = sw
    name, ns, ks, brs = chains(32)[0]
    ch = WidthsChain(rt, 2, 16, ns, ks, brs, 5)
    before = rt.chain_skinny_split_stats(), rt.chain_skinny_stats()
    rt.set_chain_skinny_split(4)
    ran_on, got = run_chain(rt, ch)
    rt.set_chain_skinny_split(0)
    ran_off, want = run_chain(rt, ch)
    assert ran_on == ran_off and (rt.chain_skinny_split_stats(), rt.chain_skinny_stats()) == before
    same_bits(got, want, "chain_skinny at 0")


def test_a_stream_without_a_scratch_block_runs_the_unsplit_launch(sw):
    """the kernel file keeps its own list of 16 scratch blocks (split_scratch.h): with the default stream's and 16 fresh streams the last one has
    none - its launch is the unsplit chain's on the same G, with that form's bits and the split counter still. (Last in the file: the list
    is full from here on.)"""
    rt, bn, P, m = sw, 32, 2, 17
    ns, ks, brs = [3 * bn + 8, 2 * bn], [128, 3 * bn + 8], [1, 1]
    ch = WidthsChain(rt, 2, m, ns, ks, brs, 23)
    # layer 0 has four steps whose sums are 0, X, -X, 1 with X = 2^26: four waves add them as ((0 + X) - X) + 1 = 1, two parts of two waves as
    # (0 + X) + (-X + 1) = 0 - bf16 rounding would hide the forms' difference on random operands
    X = ch.x.reshape(m + GUARD_ROWS, ch.ld_in[0])
    W = ch.W[0].reshape(-1, ch.ldb[0], 2)
    X[:m, :128], W[:64, :ns[0], :] = 0, 0
    for k, a, b in ((32, 8192.0, 8192.0), (64, 8192.0, -8192.0), (96, 1.0, 1.0)):
        X[:m, k], W[k // 2, :ns[0], k % 2] = orc.f32_to_bf16(np.float32([a]))[0], orc.f32_to_bf16(np.float32([b]))[0]
    ch.dx, ch.dW[0] = dev(ch.x), dev(ch.W[0])
    _, units, _, _, _ = schedule(bn, 32, P, ns, ks, brs)
    want_unsplit, want_split = one_by_one(rt, ch, bn), split_one_by_one(rt, ch, bn, P)
    assert not all(np.array_equal(a, b) for a, b in zip(want_unsplit, want_split)), "the two forms must differ in some bit for this test to see anything"
    same_bits(run_split(rt, ch, bn, P), want_split, "the default stream")
    torch.cuda.synchronize()
    moved = []
    for s in [torch.cuda.Stream() for _ in range(16)]:
        outs = ch.outputs()
        torch.cuda.synchronize()
        before, cbefore = rt.chain_skinny_split_stats()[0], rt.chain_skinny_stats()[0]
        rt.set_chain_skinny(bn), rt.set_chain_skinny_split(P)
        try:
            rt.set_stream(s)
            ran = rt.fused_brgemm_chain(BF16, ch.calls(outs))
            rt.synchronize()
        finally:
            rt.set_stream(None)
            rt.set_chain_skinny_split(0), rt.set_chain_skinny(0)
        s.synchronize()
        got = ch.host(outs)
        ch.check_windows(got)
        moved.append(rt.chain_skinny_split_stats()[0] - before)
        assert ran and rt.chain_skinny_stats() == (cbefore + 1, min(units, cus()), bn, KIND[2]), "one launch of the chain form on the split's G"
        same_bits(got, want_split if moved[-1] else want_unsplit, "stream %d" % len(moved))
    assert moved[0] == 1 and moved[-1] == 0 and moved == sorted(moved, reverse=True), moved
