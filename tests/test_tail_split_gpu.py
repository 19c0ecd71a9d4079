"""The tail split (include/tpp_xsmm_abi.h xsmm_hip_set_tail_split) on a real MI355X: a whole-layer f32 call of q CUs + r tiles, 0 < r <=
CUs / 2, as ONE launch whose q CUs body tiles run unsplit and whose r tail tiles are K-split over the idle CUs.

Shapes come from the device's CU count: 16 tile rows and CUs / 16 + extra tile columns of the forced K-split tile (variant 6: 64x64 +
K2, 7: 64x32 + K4, 9: 32x32 + K4), so that exactly one round of tiles is body and r = 16 extra tiles are tail.
  1 exact inputs (tests/exact_data.py): every tile bit for bit the oracle's, whatever the split; the launch reports "tail split" and the
    counters hold the planned tail tiles, workgroups per tail tile and body tiles
  2 random operands: every tile-sized block has the bits of today's unsplit launch or of today's split launch with the same count,
    at most r blocks differ from the former and at most the body from the latter; the whole output within the f32 bars
  3 the same call three times: identical bits - also under strict mode, in a process of its own
  4 poisoned memory around the operands and the output
  5 a forced split count takes precedence: the launch is what it is today and the counters do not move
  6 ineligible shapes under the model: the kernel and the bits of setting 0
Every case resets the setting to 0."""
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
from oracle import pyoracle as orc
from tail_split_worker import layer_call, operands
from test_parity_gpu import F32, check_close, gemm_case

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = {6: (64, 64), 7: (64, 32), 9: (32, 32)}      # forced variant -> output tile
TILE_US = {6: 0.92, 7: 0.46, 9: 0.213}              # the planner's time per 64-k chunk (gemm_plan.cpp)
HANDOFF_US = 3.5


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def shape(variant, frac):
    """(m, n, tail tiles, body tiles): 16 x (CUs / 16 + extra) tiles with r = 16 extra = CUs / frac tail tiles"""
    cus = cu_count()
    if cus % 16 or cus // frac < 16 or (cus // frac) % 16:
        pytest.skip("%d compute units do not divide into 16 tile rows with CUs / %d tail tiles" % (cus, frac))
    bm, bn = TILE[variant]
    r = cus // frac
    return 16 * bm, (cus // 16 + r // 16) * bn, r, cus


def model_split(variant, r, chunks):
    """mode 1, restated from the issue: S = min(CUs / r, 16, chunks / 4), used if S >= 2 and the saved K-loop time exceeds the hand-off"""
    S = min(cu_count() // r, 16, chunks // 4)
    if S < 2 or TILE_US[variant] * (chunks - -(-chunks // S)) <= HANDOFF_US:
        return 1
    return S


# (tail fraction of the CUs, setting): every forced count with r S <= CUs, and the model
SETTINGS = [(2, 2), (2, 1), (4, 2), (4, 4), (4, 1), (16, 2), (16, 4), (16, 16), (16, 1)]
EPILOGUES = {"beta0": dict(beta0=True), "beta1_bias_relu": dict(bias=True, relu=True),
             "strided": dict(beta0=True, bias=True, strided=True)}


def k_for(variant, setting):
    """the reduction length (k * br, 256 .. 4096): the least that gives the forced count its chunks, or lets the model split"""
    if setting == 1:
        return {6: 512, 7: 1024, 9: 4096}[variant]
    return 1024 if setting == 16 else 256


@pytest.mark.parametrize("ep", sorted(EPILOGUES))
@pytest.mark.parametrize("frac,setting", SETTINGS, ids=lambda v: str(v))
@pytest.mark.parametrize("variant", [6, 7, 9])
def test_exact_inputs_bit_for_bit_against_the_oracle(rt, variant, frac, setting, ep):
    m, n, r, body = shape(variant, frac)
    K = k_for(variant, setting)
    chunks = K // 64
    S = model_split(variant, r, chunks) if setting == 1 else min(setting, 16, chunks)
    assert S >= 2 and r * S <= cu_count(), "the case list must give every case a tail split"
    kw = dict(EPILOGUES[ep])
    if kw.pop("strided", False):
        kw.update(lda=K + 8, ldb=n + 4, ldc=n + 4, sb=64 * (n + 4), offs=(4, 8, 4, 1))
    else:
        kw.update(lda=K, ldb=n, sb=64 * n)
    before = rt.tail_split_stats()
    assert rt.set_tail_split(setting) == 0
    try:
        gemm_case(rt, F32, m, n, 64, chunks, sa=64, values="exact", ranges=ed.exact_ranges(F32, K), force=variant,
                  seed=1000 * variant + 10 * frac + setting, **kw)
        refined, after = rt.last_refined_kernel(), rt.tail_split_stats()
    finally:
        rt.set_tail_split(0)
    assert "tail split" in refined, refined
    assert after[0] == before[0] + 1
    assert after[1:] == (r, S, body), (after, (r, S, body))


def oracle_layer(m, n, K, A, B, C, D, beta0, bias, relu):
    ref, mag = C.copy(), (np.zeros_like(C) if beta0 else np.abs(C))
    flags = 4 if beta0 else 0
    orc.fused_brgemm(F32, m, n, 64, K, n, n, 64, 64 * n, flags, 0, 5 if relu else 0, 4 if bias else 0, 1 if bias else 0, A, 0, B, 0, ref, 0, D, 0, K // 64)
    orc.fused_brgemm(F32, m, n, 64, K, n, n, 64, 64 * n, flags, 0, 0, 4 if bias else 0, 1 if bias else 0, np.abs(A), 0, np.abs(B), 0, mag, 0,
                     np.abs(D), 0, K // 64)
    return ref, mag


def blocks_differ(x, y, m, n, bm, bn):
    """per output tile: do the two results differ in any bit"""
    d = (x.view(np.uint32) != y.view(np.uint32)).reshape(m // bm, bm, n // bn, bn)
    return d.any(axis=(1, 3))


@pytest.mark.parametrize("frac,setting", [(2, 2), (4, 4), (16, 16), (2, 1), (16, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("variant", [6, 7, 9])
def test_random_operands_tile_by_tile_against_the_unsplit_and_the_split_launch(rt, variant, frac, setting):
    m, n, r, body = shape(variant, frac)
    bm, bn = TILE[variant]
    K = max(k_for(variant, setting), 512)
    chunks = K // 64
    S = model_split(variant, r, chunks) if setting == 1 else min(setting, 16, chunks)
    assert S >= 2
    beta0 = setting != 1
    ep = dict(beta0=beta0, bias=True, relu=not beta0)
    A, B, C, D = operands(m, n, K, 7 * variant + frac + setting)
    try:
        rt.set_tail_split(0)
        plain, refined_plain = layer_call(rt, variant, m, n, K, A, B, C, D, **ep)
        assert refined_plain == ""
        split = None
        if m * n * S <= 8 << 20:  # the whole grid on S workgroups per tile fits the scratch block
            rt.force_split(S)
            try:
                split, refined_split = layer_call(rt, variant, m, n, K, A, B, C, D, **ep)
            finally:
                rt.force_split(-1)
            assert refined_split.endswith(", split"), refined_split
        rt.set_tail_split(setting)
        got, refined = layer_call(rt, variant, m, n, K, A, B, C, D, **ep)
    finally:
        rt.force_split(-1)
        rt.set_tail_split(0)
    assert "tail split" in refined, refined
    vs_plain = blocks_differ(got, plain, m, n, bm, bn)
    print("tail split %s: %d of %d tiles differ from the unsplit launch (tail tiles %d)" % (refined, int(vs_plain.sum()), vs_plain.size, r))
    assert vs_plain.sum() <= r
    if split is not None:
        vs_split = blocks_differ(got, split, m, n, bm, bn)
        print("  %d tiles differ from the split launch (body tiles %d)" % (int(vs_split.sum()), body))
        assert not (vs_plain & vs_split).any(), "a tile that has neither the unsplit nor the split launch's bits"
        assert vs_split.sum() <= body
    ref, mag = oracle_layer(m, n, K, A, B, C, D, **ep)
    check_close(got, ref, F32, "tail split %s m%d n%d K%d" % (refined, m, n, K), mag, K)


@pytest.mark.parametrize("variant", [6, 7, 9])
def test_three_calls_give_identical_bits_also_in_strict_mode(rt, variant):
    m, n, r, body = shape(variant, 2)
    K = k_for(variant, 1)
    A, B, C, D = operands(m, n, K, 40 + variant)
    digests = []
    try:
        assert rt.set_tail_split(1) == 0
        for _ in range(3):
            got, refined = layer_call(rt, variant, m, n, K, A, B, C, D)
            assert "tail split" in refined, refined
            digests.append(hashlib.sha256(got.view(np.uint32).tobytes()).hexdigest())
    finally:
        rt.set_tail_split(0)
    assert len(set(digests)) == 1, digests
    # strict mode is chosen before anything is queued: a fresh child process (the setting arrives through the environment there)
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_STRICT", "TPP_HIP_TAIL_SPLIT", "TPP_HIP_SPLIT")}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_TAIL_SPLIT="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tail_split_worker.py")] + [str(x) for x in (variant, m, n, K, 40 + variant)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1 and d["tail_split_from_env"] == 1
    assert all("tail split" in k for k in d["kernels"]), d["kernels"]
    assert d["stats"] == [3, r, model_split(variant, r, K // 64), body]
    assert set(d["digests"]) == set(digests), "strict mode takes the same decision: the same bits"


@pytest.mark.parametrize("variant", [6, 7, 9])
def test_poisoned_surroundings(rt, variant):
    m, n, r, body = shape(variant, 4)
    K = 512
    before = rt.tail_split_stats()
    try:
        rt.set_tail_split(4)
        gemm_case(rt, F32, m, n, 64, K // 64, lda=K + 8, ldb=n + 4, ldc=n + 4, sa=64, sb=64 * (n + 4), offs=(4, 8, 4, 1), bias=True, relu=True,
                  values="exact", ranges=ed.exact_ranges(F32, K), force=variant, poison=True, seed=variant)
        gemm_case(rt, F32, m, n, 64, K // 64, lda=K + 8, ldb=n + 4, ldc=n + 4, sa=64, sb=64 * (n + 4), offs=(4, 8, 4, 1), beta0=True, bias=True,
                  values="exact", ranges=ed.exact_ranges(F32, K), force=variant, poison=True, seed=variant + 1)
        refined, after = rt.last_refined_kernel(), rt.tail_split_stats()
    finally:
        rt.set_tail_split(0)
    assert "tail split" in refined and after == (before[0] + 2, r, 4, body)


def test_a_forced_split_count_takes_precedence(rt):
    m, n, r, body = shape(6, 2)
    K = 512
    A, B, C, D = operands(m, n, K, 5)
    plain, refined = layer_call(rt, 6, m, n, K, A, B, C, D)
    assert refined == ""
    before = rt.tail_split_stats()
    try:
        rt.set_tail_split(1)
        for forced in (0, 2):
            rt.force_split(forced)
            want, want_refined = None, None
            rt.set_tail_split(0)
            want, want_refined = layer_call(rt, 6, m, n, K, A, B, C, D)   # what the launch is today
            rt.set_tail_split(1)
            got, refined = layer_call(rt, 6, m, n, K, A, B, C, D)
            assert refined == want_refined and "tail" not in refined, (forced, refined, want_refined)
            assert refined == ("" if forced == 0 else "brgemm_f32_lw<64x64,k2>, split")
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    finally:
        rt.force_split(-1)
        rt.set_tail_split(0)
    assert rt.tail_split_stats() == before


def test_ineligible_shapes_are_untouched(rt):
    cus = cu_count()
    cases = [("one round (C2)", -1, 1024, 1024, 1024),
             ("skinny", -1, 128, 1024, 4096)]
    if cus % 16 == 0:  # three rounds minus one tile row of 64x64 tiles: r = CUs - 16 > CUs / 2
        cases.append(("three rounds minus one tile row", 6, 16 * 64, (3 * cus // 16 - 1) * 64, 512))
    for what, variant, m, n, K in cases:
        A, B, C, D = operands(m, n, K, 11)
        before = rt.tail_split_stats()
        try:
            rt.set_tail_split(0)
            want, want_refined = layer_call(rt, variant, m, n, K, A, B, C, D)
            rt.set_tail_split(1)
            got, refined = layer_call(rt, variant, m, n, K, A, B, C, D)
        finally:
            rt.set_tail_split(0)
        assert refined == want_refined and "tail" not in refined, (what, refined, want_refined)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
        assert rt.tail_split_stats() == before, what
