"""Skinny-batch f32 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_skinny_f32) on a real MI355X: with the switch on, an f32 chain with
1 <= m <= 31 rows runs as ONE launch of brgemm_f32_skinny_chain<BN, MB> with the bits of the same calls one by one under
xsmm_hip_set_skinny_f32(BN), split off. Every case runs under a forced BN (16, 32, 64) and leaves every switch 0. Buffers:
chain_widths_worker.WidthsChain(dtype=F32) - guard rows and gap columns around everything, NaN around the inputs and inside the outputs, a
sentinel around them, checked after every run. The chains are chains() below (the same list the CPU walk takes). Nothing tries to starve a
launch. As a program (a fresh process: strict mode and the switch come from the environment) it runs the eligible chain of STAYS and prints
one JSON line."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chain_edge_worker import BF16, F32, GUARD_ROWS, dev, digest
from chain_widths_worker import WidthsChain
from test_chain_skinny_f32_cpu import chains
from test_chain_switches_gpu import counters, switches

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = [1, 16, 17, 31]
BNS = [16, 32, 64]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def all_off(rt):
    switches(rt, 0)
    rt.set_chain_skinny_f32(0), rt.set_chain_skinny(0), rt.set_skinny_f32(0), rt.set_skinny_f32_split(0), rt.set_skinny_bf16(0)


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
    """every other counter a skinny f32 chain launch must leave alone"""
    return counters(rt), rt.chain_skinny_stats(), rt.skinny_f32_stats(), rt.skinny_f32_split_stats(), rt.skinny_bf16_stats(), rt.edge_tiles_stats()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_chain(rt, ch, outs=None):
    """one chain invoke on fresh (or refilled) outputs: (ran as one launch, the layers on the host), windows checked"""
    outs = ch.outputs() if outs is None else (ch.refill(outs), outs)[1]
    ran = bool(rt.fused_brgemm_chain(ch.dtype, ch.calls(outs)))
    got = ch.host(outs)
    ch.check_windows(got)
    return ran, got


def run_taken(rt, ch, mode, bn, G=None, outs=None):
    """the chain under `mode`: one launch, the new counter moved by one and holds (G, BN, waves), no other counter moved"""
    G = min(max(-(-n // bn) for n in ch.ns), cus()) if G is None else G
    waves = max(min(8, br * -(-k // 16)) for k, br in zip(ch.ks, ch.brs))
    rt.set_chain_skinny_f32(mode)
    before, o = rt.chain_skinny_f32_stats(), others(rt)
    ran, got = run_chain(rt, ch, outs)
    rt.set_chain_skinny_f32(0)
    assert ran, "the chain ran call by call"
    assert rt.chain_skinny_f32_stats() == (before[0] + 1, G, bn, waves), (before, rt.chain_skinny_f32_stats())
    assert others(rt) == o, "another counter moved"
    return got


def run_stays(rt, ch, mode):
    """the chain under `mode` with the new counter still: (ran as some other launch, the layers)"""
    rt.set_chain_skinny_f32(mode)
    before = rt.chain_skinny_f32_stats()
    ran, got = run_chain(rt, ch)
    rt.set_chain_skinny_f32(0)
    assert rt.chain_skinny_f32_stats() == before, (before, rt.chain_skinny_f32_stats())
    return ran, got


def one_by_one(rt, ch, bn, outs=None):
    """the same calls one by one on the skinny f32 kernel of the same BN, split off"""
    outs = ch.outputs() if outs is None else (ch.refill(outs), outs)[1]
    rt.set_skinny_f32(bn)
    before = rt.skinny_f32_stats()[0]
    ch.one_by_one(outs)
    got = ch.host(outs)
    rt.set_skinny_f32(0)
    assert rt.skinny_f32_stats()[0] == before + ch.L, "a reference call did not run on the skinny f32 kernel"
    return got


def same_bits(got, want, what):
    for l, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), "%s: layer %d differs" % (what, l)


def check_exact(ch, got):
    """every layer bit for bit the fp64 result of the fp64 previous layer cast to f32; the precondition - every value an integer below
    2^24 in magnitude, so that every partial sum in any order is exact - is asserted"""
    rows, cur = ch.m + GUARD_ROWS, ch.x.reshape(ch.m + GUARD_ROWS, -1)[:ch.m].astype(np.float64)
    for l in range(ch.L):
        K, n = ch.ks[l] * ch.brs[l], ch.ns[l]
        w = ch.W[l].reshape(-1, ch.ldb[l])[:K, :n].astype(np.float64)
        assert (np.abs(cur[:, :K]) @ np.abs(w) + np.abs(ch.b[l][:n])).max() < 2 ** 24, "layer %d not exact" % l
        cur = np.maximum(cur[:, :K] @ w + ch.b[l][:n].astype(np.float64)[None, :], 0)
        g = got[l].reshape(rows, ch.ldc[l])[:ch.m, :n]
        bad = g.view(np.uint32) != cur.astype(np.float32).view(np.uint32)
        assert not bad.any(), "layer %d: %d elements differ from fp64, first at (row, column) %s" % (l, int(bad.sum()), tuple(np.argwhere(bad)[0]))


@pytest.mark.parametrize("bn", BNS)
def test_exact_inputs_every_layer_bit_for_bit_fp64(sw, bn):
    for name, ns, ks, brs in chains(bn)[:5]:
        for m in MS:
            ch = WidthsChain(sw, 0, m, ns, ks, brs, 31 * m + bn + len(name), exact=True, dtype=F32)
            check_exact(ch, run_taken(sw, ch, bn, bn))


@pytest.mark.parametrize("G", [1, 3, 7])
@pytest.mark.parametrize("bn", BNS)
def test_a_forced_group_count_walks_the_blocks(sw, bn, G):
    name, ns, ks, brs = chains(bn)[5]  # 7 blocks, the last one shifted back
    for m in (16, 31):
        ch = WidthsChain(sw, 0, m, ns, ks, brs, m + bn + G, exact=True, dtype=F32)
        check_exact(ch, run_taken(sw, ch, 1000 * G + bn, bn, G))


@pytest.mark.parametrize("bn", BNS)
def test_six_steps_back_to_back_equal_the_calls_one_by_one(sw, bn):
    rt, steps = sw, 6
    rt.set_stream(torch.cuda.current_stream())  # (the stream torch's copies below are queued on)
    for name, ns, ks, brs in chains(bn)[:4]:
        for m in MS:
            ch = WidthsChain(rt, 0, m, ns, ks, brs, 77 + 31 * m + bn + len(name), dtype=F32)
            rng, k, x0, xs = np.random.default_rng(m + bn), ks[0] * brs[0], ch.dx, []
            for _ in range(steps):  # other layer-0 inputs: a stale line of the previous step would show
                X = ch.x.copy().reshape(m + GUARD_ROWS, ch.ld_in[0])
                X[:m, :k] = rng.uniform(-1, 1, (m, k)).astype(np.float32)
                xs.append(dev(X.reshape(-1)))
            outs, want = ch.outputs(), []
            for x in xs:
                ch.dx = x
                want.append(one_by_one(rt, ch, bn, outs))
            ch.dx = x0
            run_taken(rt, ch, bn, bn)  # (the block's first launch is followed by a synchronisation: not in the loop below)
            for rep in range(3):
                ch.refill(outs)
                rt.set_chain_skinny_f32(bn)
                stash, ran = [], []
                for x in xs:  # no synchronisation in here: the copies are stream-ordered behind each launch
                    ch.dx = x
                    ran.append(rt.fused_brgemm_chain(F32, ch.calls(outs)))
                    stash.append([o.clone() for o in outs])
                rt.set_chain_skinny_f32(0)
                ch.dx = x0
                rt.synchronize()
                torch.cuda.synchronize()
                assert all(ran), ran
                for step, s in enumerate(stash):
                    got = [o.cpu().numpy() for o in s]
                    ch.check_windows(got)
                    same_bits(got, want[step], "%s m %d repeat %d step %d" % (name, m, rep, step))


@pytest.mark.parametrize("where", ["A", "B"])
@pytest.mark.parametrize("bn", BNS)
def test_an_inf_in_the_ragged_tail_counts_once(sw, bn, where):
    """k0 = 36: the last step keeps one lane group (k = 32 .. 35). Layer 0's operands positive integers, one +Inf at k = 33: +Inf in exactly
    its row (A) or column (B) of layer 0, no NaN - a zero on one side only, or a load beyond k, would show"""
    rt = sw
    name, ns, ks, brs = chains(bn)[0]
    k, n = ks[0], ns[0]
    for m in (16, 31):
        ch = WidthsChain(rt, 0, m, ns, ks, brs, m + bn, exact=True, dtype=F32)
        rng = np.random.default_rng(m + bn)
        X, W = ch.x.reshape(m + GUARD_ROWS, ch.ld_in[0]), ch.W[0].reshape(-1, ch.ldb[0])
        X[:m, :k], W[:k, :n] = rng.integers(1, 4, (m, k)), rng.integers(1, 4, (k, n))
        want = np.zeros((m, n), bool)
        if where == "A":
            X[m - 1, 33], want[m - 1, :] = np.inf, True
        else:
            W[33, n - 3], want[:, n - 3] = np.inf, True
        ch.dx, ch.dW[0] = dev(ch.x), dev(ch.W[0])
        rt.set_chain_skinny_f32(bn)
        outs = ch.outputs()
        ran = rt.fused_brgemm_chain(F32, ch.calls(outs))
        got = ch.host(outs)
        rt.set_chain_skinny_f32(0)
        g = got[0].reshape(m + GUARD_ROWS, ch.ldc[0])[:m, :n]
        assert ran and not np.isnan(g).any(), "call by call, or a NaN: an Inf met a one-sided zero, or memory beyond k was read"
        assert np.array_equal(np.isposinf(g), want) and not np.isneginf(g).any()
        same_bits(got, one_by_one(rt, ch, bn), "m %d" % m)


def test_an_f32_and_a_bf16_skinny_chain_share_a_counter_block(sw):
    """both are keyed (stream, 1, G = 2, 2 layers) and add 2 to the one seam counter per launch"""
    rt, bn = sw, 32
    a = WidthsChain(rt, 0, 16, [3 * bn + 4, 2 * bn], [36, 3 * bn + 4], [1, 1], 811, dtype=F32)
    b = WidthsChain(rt, 2, 16, [3 * bn + 8, 2 * bn], [72, 3 * bn + 8], [1, 1], 812)
    alone_a = run_taken(rt, a, 2000 + bn, bn, 2)
    rt.set_chain_skinny(2000 + bn)
    before = rt.chain_skinny_stats()[0]
    ran_b, alone_b = run_chain(rt, b)
    assert ran_b and rt.chain_skinny_stats()[0] == before + 1
    outs_a, outs_b = a.outputs(), b.outputs()
    rt.set_chain_skinny_f32(2000 + bn)
    ran = [rt.fused_brgemm_chain(ch.dtype, ch.calls(o)) for _ in range(3) for ch, o in ((a, outs_a), (b, outs_b))]  # no synchronisation in between
    got_a, got_b = a.host(outs_a), b.host(outs_b)
    assert all(ran)
    same_bits(got_a, alone_a, "the f32 chain")
    assert all(np.array_equal(g, w) for g, w in zip(got_b, alone_b)), "the bf16 chain"


# (what, m, n per layer, k per layer, the mode asked for, keyword arguments of WidthsChain)
STAYS = [("a bf16 chain", 16, [72, 64], [64, 72], 32, dict(dtype=BF16)),
         ("m = 32", 32, [72, 64], [64, 72], 32, {}),
         ("n % 4 != 0", 16, [70, 64], [64, 68], 32, {}),
         ("k % 4 == 2", 16, [72, 64], [66, 72], 32, {}),
         ("some n_l < BN", 16, [72, 32, 64], [64, 72, 32], 64, {})]


def eligible(rt, seed=9):
    return WidthsChain(rt, 0, 16, [72, 64], [64, 72], [1, 1], seed, exact=True, dtype=F32)


@pytest.mark.parametrize("what,m,ns,ks,mode,kw", STAYS, ids=[s[0] for s in STAYS])
def test_chains_that_stay_call_by_call(sw, what, m, ns, ks, mode, kw):
    ch = WidthsChain(sw, 2 if kw else 0, m, ns, ks, [1] * len(ns), 9, exact=True, **(kw or dict(dtype=F32)))
    (ran_off, want), (ran_on, got) = run_stays(sw, ch, 0), run_stays(sw, ch, mode)
    assert ran_on == ran_off, what
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)), what


def test_beta_1_and_synchronous_mode_stay_and_the_eligible_chain_is_taken(sw):
    rt = sw
    ch = eligible(rt)
    check_exact(ch, run_taken(rt, ch, 32, 32, 3))
    _, want = run_stays(rt, ch, 0)
    rt.set_async(False)
    ran, got = run_stays(rt, ch, 32)
    rt.set_async(True)
    assert not ran and all(np.array_equal(g, w) for g, w in zip(got, want))
    l = 1  # call 1 accumulates into its output: the template's window holds zeros instead of NaN
    ch.handles[l] = rt.fused_brgemm_dispatch(F32, ch.m, ch.ns[l], ch.ks[l], ch.ld_in[l], ch.ldb[l], ch.ldc[l], ch.ks[l], ch.ks[l] * ch.ldb[l], ch.flags & ~4, 0, 5, 4, 1)
    ch.out_templates[l].reshape(ch.m + GUARD_ROWS, ch.ldc[l])[:ch.m, :ch.ns[l]] = 0
    ch.d_templates[l] = dev(ch.out_templates[l])
    (_, want), (ran, got) = run_stays(rt, ch, 0), run_stays(rt, ch, 32)
    assert not ran and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_strict_mode_in_a_child_process_stays(sw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}
    env.update(TPP_HIP_CHAIN_SKINNY_F32="32", TPP_HIP_STRICT="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["mode_from_env"] == 32, d
    assert d["ran_as_one"] is False and d["ran_as_one_off"] is False and d["stats"][0] == 0 and d["digests"] == d["digests_off"], d
    assert d["digests"] == [digest(g) for g in run_taken(sw, eligible(sw), 32, 32, 3)], "exact data: the strict child's bits are the launch's"


def test_a_batch_8_f32_mlp_through_sharded_mlp_is_one_launch(sw):
    """MlpSpec(batch 8, layers 256 -> 200 -> 256 -> 64, f32), bias + relu: call by call today; under a forced BN 16 one launch per step
    with the bits of the call-by-call step under set_skinny_f32(16)"""
    rt = sw
    spec = pkg.MlpSpec(batch=8, layers=[256, 200, 256, 64], dtype=F32)
    rng = np.random.default_rng(3)
    dx = dev(rng.uniform(-1, 1, 8 * 256).astype(np.float32))
    dw = [dev(rng.uniform(-0.5, 0.5, k * n).astype(np.float32)) for k, n in zip(spec.layers[:-1], spec.layers[1:])]
    db = [dev(rng.uniform(-1, 1, n).astype(np.float32)) for n in spec.layers[1:]]
    mlp = pkg.ShardedMlp(spec, rt=rt)

    def step():
        acts = [torch.full((8 * n,), float("nan"), device="cuda") for n in spec.layers[1:]]
        out = mlp.forward(dx, dw, db, acts)
        rt.synchronize()
        torch.cuda.synchronize()
        assert out is acts[-1]
        return [a.cpu().numpy() for a in acts]
    rt.set_skinny_f32(16)
    want = step()
    rt.set_skinny_f32(0)
    assert mlp.last_step_fused is False
    rt.set_chain_skinny_f32(16)
    before = rt.chain_skinny_f32_stats()
    got = [step() for _ in range(3)]
    fused = mlp.last_step_fused
    rt.set_chain_skinny_f32(0)
    assert fused is True and rt.chain_skinny_f32_stats() == (before[0] + 3, min(16, cus()), 16, 8), rt.chain_skinny_f32_stats()
    for g in got:
        same_bits(g, want, "the one launch against the call-by-call step")


if __name__ == "__main__":
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    mode = rt.set_chain_skinny_f32(0)
    rt.set_chain_skinny_f32(mode)
    out = {"strict": rt.get_strict(), "mode_from_env": mode}
    ch = eligible(rt)
    ran, got = run_chain(rt, ch)
    out["ran_as_one"], out["digests"], out["stats"] = ran, [digest(g) for g in got], list(rt.chain_skinny_f32_stats())
    rt.set_chain_skinny_f32(0)
    ran, got = run_chain(rt, ch)
    out["ran_as_one_off"], out["digests_off"] = ran, [digest(g) for g in got]
    rt.set_async(was_async)
    print(json.dumps(out))
