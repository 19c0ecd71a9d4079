"""Skinny-batch bf16 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_skinny) on a real MI355X: with the switch on, a bf16 chain with
1 <= m <= 31 rows runs as ONE launch of brgemm_bf16_skinny_chain<IMG, BN, MB> - G resident workgroups, workgroup w computing the column blocks
w, w + G, .. of every layer, one counter per seam - with the bits of the same calls one by one under xsmm_hip_set_skinny_bf16(BN).

Every case runs under a forced BN (16, 32, 64; every (image, BN) that has an instance) and leaves every switch 0. Buffers:
chain_widths_worker.WidthsChain - 8 guard rows and 8 gap columns around everything, NaN around the inputs and inside the outputs, a
sentinel around them, checked after every run. m in {1, 16, 17, 31}. The chains (n per layer; BN = the column-block width):
  ragged k        [3 BN + 8] * 3, k0 = 72: a ragged k, a shifted last block, W_0 = 3 waves against the later layers' own
  sit out         [4 BN, BN, 2 BN + 8]: workgroups 1 .. 3 sit layer 1 out (they arrive at once) and resume
  waves 1 / 8     [264, 72, BN] with k = [32, 264, 32]: W = 1, 8, 1
  batches         [144, 96, 64] with (k, br) = (40, 2), (72, 2), (32, 3): batch elements walking along k
  eight layers    [2 BN + 8, BN + 8] * 4
  forced G        [6 BN + 8] * 2 (7 blocks) under 1000 * G + BN with G = 1, 3 (the block walk 0, 3, 6) and 7
  1 exact inputs, bias + relu: every layer bit for bit the oracle's (check_exact asserts its own precondition); one launch, the new
    counter moved by one with G, BN and the image, no other chain or single-call counter moved
  2 random operands, six steps back to back on the SAME output buffers with no synchronisation in between, each with another layer-0
    input (a stale line of the previous step would show): every step equals the same calls one by one under set_skinny_bf16(BN), split
    off. No tolerance. Three repeats, identical bits
  3 one +Inf in A, or in a weight, at a k of the ragged tail (k0 = 72, k = 67) counts once
  4 a skinny chain (G = 2, two layers) and a plain chain (32 rows x [128, 128] of flat B on the 32x64 tile: one row block, two column tiles) share a
    counter block and alternate three times each on one stream: each has the bits it has alone
  5 what stays call by call, with the bits of the switch-off run and the counter still
  6 with the new switch on, one m >= 32 chain per existing form answers as with it off
  7 ShardedMlp(MlpSpec(batch=8, layers=[256, 200, 256, 64])): last_step_fused, the bits of the call-by-call step
Nothing tries to starve a launch."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chain_edge_worker import BASE, BF16, F32, GUARD_ROWS, dev, digest, orc
from chain_skinny_worker import KIND, groups, instance_exists, run_chain
from chain_widths_worker import WidthsChain, check_exact
from test_chain_switches_gpu import CASES as FORM_CASES
from test_chain_switches_gpu import counters, layers, switches

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = [1, 16, 17, 31]
INSTANCES = [(image, bn) for image in (2, 0, 4) for bn in (16, 32, 64) if instance_exists(image, bn)]
INF = 0x7F80


def chains(bn):
    """(id, n per layer, k per layer, batch per layer)"""
    return [("ragged_k", [3 * bn + 8] * 3, [72, 3 * bn + 8, 3 * bn + 8], [1, 1, 1]),
            ("sit_out", [4 * bn, bn, 2 * bn + 8], [64, 4 * bn, bn], [1, 1, 1]),
            ("waves_1_8", [264, 72, bn], [32, 264, 32], [1, 1, 1]),
            ("batches", [144, 96, 64], [40, 72, 32], [2, 2, 3]),
            ("eight_layers", [2 * bn + 8, bn + 8] * 4, [64] + [2 * bn + 8, bn + 8] * 3 + [2 * bn + 8], [1] * 8)]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def all_off(rt):
    switches(rt, 0)
    rt.set_chain_skinny(0), rt.set_skinny_bf16(0), rt.set_skinny_split(0)


@pytest.fixture()
def sw(rt):
    """asynchronous mode for the case; whatever happens, every switch is 0 afterwards"""
    was_async = rt.set_async(True)
    all_off(rt)
    try:
        yield rt
    finally:
        rt.synchronize()
        all_off(rt)
        rt.set_async(was_async)


def others(rt):
    """every other counter a skinny chain launch must leave alone"""
    return (counters(rt), rt.skinny_bf16_stats(), rt.skinny_split_stats(), rt.edge_tiles_stats(), rt.edge_k_bf16_stats(), rt.edge_k8_bf16_stats(),
            rt.dma256_images_stats(), rt.dma256_edge_stats())


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_taken(rt, ch, mode, G, bn, outs=None):
    """the chain under `mode`: one launch, the new counter moved by one and describes it, no other counter moved"""
    rt.set_chain_skinny(mode)
    before, o = rt.chain_skinny_stats(), others(rt)
    ran, got = run_chain(rt, ch, outs)
    rt.set_chain_skinny(0)
    assert ran, "the chain ran call by call"
    assert rt.chain_skinny_stats() == (before[0] + 1, G, bn, KIND[ch.image]), (before, rt.chain_skinny_stats())
    assert others(rt) == o, "another counter moved"
    return got


def run_stays(rt, ch, mode):
    """the chain under `mode`: call by call, the counter still; returns the layers"""
    rt.set_chain_skinny(mode)
    before = rt.chain_skinny_stats()
    ran, got = run_chain(rt, ch)
    rt.set_chain_skinny(0)
    assert not ran and rt.chain_skinny_stats() == before, (ran, before, rt.chain_skinny_stats())
    return got


def one_by_one(rt, ch, bn, outs=None, windows=True):
    """the same calls one by one on the skinny kernel of the same BN, split off"""
    if outs is None:
        outs = ch.outputs()
    else:
        ch.refill(outs)
    rt.set_skinny_bf16(bn)
    before = rt.skinny_bf16_stats()[0]
    ch.one_by_one(outs)
    got = ch.host(outs)
    rt.set_skinny_bf16(0)
    assert rt.skinny_bf16_stats()[0] == before + ch.L, "a reference call did not run on the skinny kernel"
    if windows:  # (not with another layer-0 input in place: check_windows compares the chain's own)
        ch.check_windows(got)
    return got


@pytest.mark.parametrize("image,bn", INSTANCES)
def test_exact_inputs_every_layer_bit_for_bit_the_oracle_s(sw, image, bn):
    rt = sw
    for name, ns, ks, brs in chains(bn):
        for m in MS:
            ch = WidthsChain(rt, image, m, ns, ks, brs, 1000 * image + 31 * m + bn + len(name), exact=True)
            got = run_taken(rt, ch, bn, groups(ns, bn, cus()), bn)
            check_exact(ch, got)


@pytest.mark.parametrize("G", [1, 3, 7])
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_a_forced_group_count_walks_the_blocks(sw, image, bn, G):
    rt = sw
    n = 6 * bn + 8  # 7 blocks, the last one shifted back
    for m in (16, 31):
        ch = WidthsChain(rt, image, m, [n, n], [72, n], [1, 1], 50 * image + m + bn + G, exact=True)
        got = run_taken(rt, ch, 1000 * G + bn, G, bn)
        check_exact(ch, got)


def variants(ch, steps, seed):
    """`steps` layer-0 inputs: the chain's own buffer with other random values inside its window"""
    rng = np.random.default_rng(seed)
    k = ch.ks[0] * ch.brs[0]
    xs = []
    for _ in range(steps):
        X = ch.x.copy().reshape(ch.m + GUARD_ROWS, ch.ld_in[0])
        X[:ch.m, :k] = orc.f32_to_bf16(rng.uniform(-1, 1, ch.m * k).astype(np.float32)).reshape(ch.m, k)
        xs.append(dev(X.reshape(-1)))
    return xs


@pytest.mark.parametrize("image,bn", INSTANCES)
def test_six_steps_back_to_back_equal_the_calls_one_by_one(sw, image, bn):
    rt = sw
    rt.set_stream(torch.cuda.current_stream())  # (the stream torch's copies below are queued on)
    steps = 6
    for name, ns, ks, brs in chains(bn)[:3]:
        for m in MS:
            ch = WidthsChain(rt, image, m, ns, ks, brs, 77 * image + 31 * m + bn + len(name))
            xs, x0 = variants(ch, steps, m + bn), ch.dx
            want = []
            outs = ch.outputs()
            for x in xs:
                ch.dx = x
                want.append(one_by_one(rt, ch, bn, outs, windows=False))
            ch.dx = x0
            run_taken(rt, ch, bn, groups(ns, bn, cus()), bn)  # (the block's first launch is followed by a synchronisation: not in the loop below)
            first = None
            for rep in range(3):
                ch.refill(outs)
                rt.set_chain_skinny(bn)
                stash, ran = [], []
                for x in xs:  # no synchronisation in here: the copies are stream-ordered behind each launch
                    ch.dx = x
                    ran.append(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
                    stash.append([o.clone() for o in outs])
                rt.set_chain_skinny(0)
                ch.dx = x0
                rt.synchronize()
                torch.cuda.synchronize()
                assert all(ran), ran
                got = [[o.cpu().numpy().view(np.uint16) for o in s] for s in stash]
                for step in range(steps):
                    ch.check_windows(got[step])
                    for l in range(ch.L):
                        assert np.array_equal(got[step][l], want[step][l]), "%s m %d repeat %d step %d layer %d differs from the calls one by one" % (name, m, rep, step, l)
                if first is None:
                    first = got
                assert all(np.array_equal(a, b) for s, f in zip(got, first) for a, b in zip(s, f)), "repeat %d differs" % rep


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("image,bn", INSTANCES)
def test_an_inf_in_the_ragged_tail_counts_once(sw, image, bn, where):
    """k0 = 72: the last step keeps one lane group (k = 64 .. 71). Layer 0's operands positive integers, one +Inf at k = 67: +Inf in exactly
    its row (A) or column (B) of layer 0, no NaN there - a zero on one side only, or a load beyond k, would show; every layer has the bits
    of the calls one by one"""
    rt = sw
    k, n, v = 72, 3 * bn + 8, image or 1
    for m in (16, 31):
        ch = WidthsChain(rt, image, m, [n, n], [k, n], [1, 1], 5 * image + m + bn, exact=True)
        rng = np.random.default_rng(m + bn)
        X = ch.x.reshape(m + GUARD_ROWS, ch.ld_in[0])
        X[:m, :k] = orc.f32_to_bf16(rng.integers(1, 4, m * k).astype(np.float32)).reshape(m, k)
        W = ch.W[0].reshape(-1, ch.ldb[0], v)
        W[:k // v, :n, :] = orc.f32_to_bf16(rng.integers(1, 4, k * n).astype(np.float32)).reshape(k // v, n, v)
        r, c, kinf = m - 1, n - 3, 67
        if where == "A":
            X[r, kinf] = INF
        else:
            W[kinf // v, c, kinf % v] = INF
        ch.dx, ch.dW[0] = dev(ch.x), dev(ch.W[0])
        rt.set_chain_skinny(bn)
        before = rt.chain_skinny_stats()[0]
        outs = ch.outputs()
        ran = rt.fused_brgemm_chain(BF16, ch.calls(outs))
        got = ch.host(outs)
        rt.set_chain_skinny(0)
        assert ran and rt.chain_skinny_stats()[0] == before + 1
        g = orc.bf16_to_f32(got[0]).reshape(m + GUARD_ROWS, ch.ldc[0])[:m, :n]
        want = np.zeros((m, n), bool)
        if where == "A":
            want[r, :] = True
        else:
            want[:, c] = True
        assert not np.isnan(g).any(), "a NaN: an Inf met a one-sided zero, or memory beyond k was read"
        assert np.array_equal(np.isposinf(g), want) and not np.isneginf(g).any()
        outs2 = ch.outputs()
        rt.set_skinny_bf16(bn)
        ch.one_by_one(outs2)
        ref = ch.host(outs2)
        rt.set_skinny_bf16(0)
        for l in range(ch.L):
            assert np.array_equal(got[l], ref[l]), "layer %d differs from the calls one by one" % l


def test_a_skinny_chain_and_a_plain_chain_share_a_counter_block(sw):
    """both are keyed (stream, 1 row block, 2 column tiles / workgroups, 2 layers) and add 2 to the one seam counter per launch"""
    rt = sw
    bn = 32
    a = WidthsChain(rt, 2, 16, [3 * bn + 8, 2 * bn], [72, 3 * bn + 8], [1, 1], 811, exact=True)
    b = WidthsChain(rt, 0, 32, [128, 128], [64, 128], [1, 1], 812, exact=True, tiles=0)  # (flat B: a VNNI-2 call on these tiles needs 64 rows)
    mode = 2000 + bn
    alone_a = run_taken(rt, a, mode, 2, bn)
    before = counters(rt)
    ran_b, alone_b = run_chain(rt, b)
    assert ran_b and counters(rt) == before, "the plain chain did not run as a plain launch"
    check_exact(a, alone_a), check_exact(b, alone_b)
    outs_a, outs_b = a.outputs(), b.outputs()
    for step in range(3):
        got_a = run_taken(rt, a, mode, 2, bn, outs_a)
        ran_b, got_b = run_chain(rt, b, outs_b)
        assert ran_b
        for l in range(2):
            assert np.array_equal(got_a[l], alone_a[l]) and np.array_equal(got_b[l], alone_b[l]), "step %d layer %d" % (step, l)
    # back to back, no synchronisation between the two forms
    a.refill(outs_a), b.refill(outs_b)
    rt.set_chain_skinny(mode)
    ran = [rt.fused_brgemm_chain(BF16, ch.calls(o)) for _ in range(3) for ch, o in ((a, outs_a), (b, outs_b))]
    rt.set_chain_skinny(0)
    got_a, got_b = a.host(outs_a), b.host(outs_b)
    assert all(ran)
    for l in range(2):
        assert np.array_equal(got_a[l], alone_a[l]) and np.array_equal(got_b[l], alone_b[l]), "back to back, layer %d" % l


# (what, image, m, n per layer, k per layer, the mode asked for, keyword arguments of WidthsChain / how the eligible chain differs)
STAYS = [("f32", 2, 16, [72, 64], [64, 72], 32, dict(dtype=F32)),
         ("m = 32", 2, 32, [72, 64], [64, 72], 32, {}),
         ("n % 8 != 0", 2, 16, [100, 64], [64, 96], 32, {}),
         ("k % 8 == 4", 2, 16, [72, 64], [68, 72], 32, {}),
         ("some n_l < BN", 2, 16, [72, 32, 64], [64, 72, 32], 64, {}),
         ("a flat B under BN 16", 0, 16, [72, 64], [64, 72], 16, {}),
         ("a forced generic kernel", 2, 16, [72, 64], [64, 72], 32, dict(tiles=8 - BASE[2])),
         ("calls that differ in m", 2, 16, [72, 64, 72], [64, 72, 64], 32, dict(ms=[16, 8, 16]))]


@pytest.mark.parametrize("what,image,m,ns,ks,mode,kw", STAYS, ids=[s[0] for s in STAYS])
def test_chains_that_stay_call_by_call(sw, what, image, m, ns, ks, mode, kw):
    rt = sw
    ch = WidthsChain(rt, image, m, ns, ks, [1] * len(ns), 9, exact=True, **kw)
    outs = ch.outputs()
    dt = kw.get("dtype", BF16)

    def run(md):
        ch.refill(outs)
        rt.set_chain_skinny(md)
        before = rt.chain_skinny_stats()
        ran = rt.fused_brgemm_chain(dt, ch.calls(outs))
        got = ch.host(outs)
        rt.set_chain_skinny(0)
        assert rt.chain_skinny_stats() == before, what
        return ran, got
    ran_off, want = run(0)
    ran_on, got = run(mode)
    assert ran_on == ran_off and (dt == F32 or m >= 32 or not ran_on), (what, ran_on, ran_off)
    assert all(np.array_equal(g, w, equal_nan=dt == F32) for g, w in zip(got, want)), what


def eligible(rt, seed=9):
    return WidthsChain(rt, 2, 16, [72, 64], [64, 72], [1, 1], seed, exact=True)


def test_the_eligible_chain_of_the_stays_list_is_taken(sw):
    run_taken(sw, eligible(sw), 32, 3, 32)


def test_the_switch_off_with_every_other_switch_on_stays(sw):
    rt = sw
    ch = eligible(rt)
    want = run_stays(rt, ch, 0)
    switches(rt, 1)
    rt.set_skinny_bf16(1), rt.set_skinny_split(1)
    before = counters(rt)
    got = run_stays(rt, ch, 0)
    assert counters(rt) == before
    all_off(rt)
    check_exact(ch, got)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_synchronous_mode_stays(sw):
    rt = sw
    ch = eligible(rt)
    want = run_stays(rt, ch, 0)
    rt.set_async(False)
    got = run_stays(rt, ch, 32)
    rt.set_async(True)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_a_beta_1_call_stays(sw):
    rt = sw
    ch = eligible(rt)
    l = 1  # call 1 accumulates into its output: the template's window holds zeros instead of NaN
    ch.handles[l] = rt.fused_brgemm_dispatch(BF16, ch.m, ch.ns[l], ch.ks[l], ch.ld_in[l], ch.ldb[l], ch.ldc[l], ch.ks[l], ch.ks[l] * ch.ldb[l], ch.flags & ~4, 0, 5, 4, 1)
    t = ch.out_templates[l].reshape(ch.m + GUARD_ROWS, ch.ldc[l])
    t[:ch.m, :ch.ns[l]] = 0
    ch.d_templates[l] = dev(ch.out_templates[l])
    want = run_stays(rt, ch, 0)
    got = run_stays(rt, ch, 32)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_strict_mode_in_a_child_process_stays(sw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}
    env.update(TPP_HIP_CHAIN_SKINNY="32", TPP_HIP_STRICT="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_skinny_worker.py"), "2", "16", "9", "72,64", "64"], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["chain_skinny_from_env"] == 32, d
    assert d["ran_as_one"] is False and d["ran_as_one_off"] is False and d["chain_skinny_stats"][0] == 0 and d["digests"] == d["digests_off"], d
    ch = eligible(sw)
    assert d["digests"] == [digest(g) for g in run_taken(sw, ch, 32, 3, 32)], "exact data: the strict child's bits are the launch's"


@pytest.mark.parametrize("name,row,m,sizes,k_all,images,width_rounds,forced_form", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_with_the_switch_on_every_existing_form_answers_as_before(sw, name, row, m, sizes, k_all, images, width_rounds, forced_form):
    rt = sw
    ns, ks = layers(sizes, k_all)
    ch = WidthsChain(rt, images[0], m, ns, ks, [1] * len(ns), 700 + len(name), exact=True)
    seen = []
    for mode in (0, 1):
        switches(rt, 1, width_rounds)
        rt.set_chain_skinny(mode)
        before, sbefore = counters(rt), rt.chain_skinny_stats()
        ran, got = run_chain(rt, ch)
        after = counters(rt)
        assert rt.chain_skinny_stats() == sbefore
        all_off(rt)
        seen.append((ran, {k: after[k] - before[k] for k in after}, [digest(g) for g in got]))
    assert seen[0] == seen[1], (name, seen[0][:2], seen[1][:2])


def test_a_batch_8_mlp_through_sharded_mlp_is_one_launch(sw):
    """MlpSpec(batch 8, layers 256 -> 200 -> 256 -> 64), bf16, bias + relu: call by call today; under the switch one launch per step with
    the bits of the call-by-call step on the skinny kernel of the same BN. Mode 1 (256 -> 200 -> 256 -> 64 at 8 rows: below the gate's 17
    rows) picks BN 16."""
    rt = sw
    spec = pkg.MlpSpec(batch=8, layers=[256, 200, 256, 64])
    rng = np.random.default_rng(3)
    bf = lambda a: orc.f32_to_bf16(np.ascontiguousarray(a, dtype=np.float32).ravel())  # noqa: E731
    x = bf(rng.uniform(-1, 1, (8, 256)))
    ws = [rng.uniform(-0.5, 0.5, (k, n)).astype(np.float32) for k, n in zip(spec.layers[:-1], spec.layers[1:])]
    wv = [bf(w.reshape(w.shape[0] // 2, 2, w.shape[1]).transpose(0, 2, 1)) for w in ws]  # VNNI-2: [k / 2][n][2]
    bs = [bf(rng.uniform(-1, 1, n)) for n in spec.layers[1:]]
    dx, dw, db = dev(x), [dev(w) for w in wv], [dev(b) for b in bs]
    mlp = pkg.ShardedMlp(spec, rt=rt)

    def step():
        acts = [torch.full((8 * n,), 0x7FC0, dtype=torch.int16, device="cuda") for n in spec.layers[1:]]
        out = mlp.forward(dx, dw, db, acts)
        rt.synchronize()
        torch.cuda.synchronize()
        assert out is acts[-1]
        return [a.cpu().numpy().view(np.uint16) for a in acts]
    rt.set_skinny_bf16(16)
    want = step()
    rt.set_skinny_bf16(0)
    assert mlp.last_step_fused is False
    rt.set_chain_skinny(1)
    before = rt.chain_skinny_stats()
    got = [step() for _ in range(3)]
    fused = mlp.last_step_fused
    rt.set_chain_skinny(0)
    assert fused is True and rt.chain_skinny_stats() == (before[0] + 3, min(16, cus()), 16, 0), rt.chain_skinny_stats()
    for g in got:
        assert all(np.array_equal(a, b) for a, b in zip(g, want)), "the one launch differs from the call-by-call step"
