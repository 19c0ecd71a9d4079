"""CPU check of the half-step bf16 ragged-k schedule (tpp-mlir_amd/csrc/brgemm_bf16_lw_kedge.h bkedge8_*, xsmm_hip_set_edge_k8_bf16): the
header the kernel, its launcher and the planner include, compiled as plain host C++ with tests/edge_k8_bf16_schedule/driver.cpp. For every
k in 72 .. 648 in steps of 16 (k % 16 == 8), 1 .. 3 batch elements and K splits 1 and 2: the k-values multiplied are exactly 0 .. k - 1 of
each batch element, each once, in ascending order - a half step counting as its upper eight; no chunk starts below 0 or ends beyond k; the
loader's steps are [64, ..., k % 64]; the shifted start is a multiple of 8 k-values; every last chunk has exactly one half step, and it
is the first step of the chunk that runs."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

KS = list(range(72, 649, 16))
STRIDE_PAD = 40  # the driver's batch stride is k + 40


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("edge_k8_bf16_schedule") / "schedule")
    # C++14: the header is for any host compiler of that standard
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "edge_k8_bf16_schedule", "driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    cases, ok, facts = {}, {}, {}
    for l in out:
        f = l.split()
        if f[0] == "ok":
            ok[int(f[1])] = int(f[2])
            continue
        if f[0] == "facts":
            facts[int(f[1])] = tuple(int(x) for x in f[2:])
            continue
        k, br, wk, b, c = (int(x) for x in f[:5])
        # a group's steps: (step, upper half only?)
        steps = [[(int(s), u == "u") for s, u in re.findall(r"(\d)(u?)", g)] for g in f[8].split(",")] if len(f) > 8 else [[]]
        cases.setdefault((k, br, wk), []).append(dict(b=b, c=c, pos=int(f[5][1:]), start=int(f[6][1:]), skip=int(f[7][1:]), steps=steps))
    return cases, ok, facts


def test_every_case_is_there(walk):
    cases, ok, facts = walk
    assert sorted(cases) == [(k, br, wk) for k in KS for br in (1, 2, 3) for wk in (1, 2)]
    assert len(KS) == 37 and all(k >= 64 and k % 16 == 8 for k in KS)
    # not taken: below a chunk, whole chunks, k % 8 != 0, the other switch's k % 16 == 0; taken: 72, 200, 1000
    assert ok == {0: 0, 8: 0, 56: 0, 64: 0, 76: 0, 80: 0, 128: 0, 784: 0, 72: 1, 200: 1, 1000: 1}
    # (chunks per element, o) of the lengths the GPU tests and the A/B run
    assert facts == {72: (2, 56), 88: (2, 40), 104: (2, 24), 120: (2, 8), 168: (3, 24), 200: (4, 56), 296: (5, 24), 568: (9, 8), 1000: (16, 24)}


def test_the_k_values_multiplied_are_each_batch_element_once_in_order(walk):
    cases, _, _ = walk
    for (k, br, wk), rows in cases.items():
        assert [(r["b"], r["c"]) for r in rows] == [(b, c) for b in range(br) for c in range(-(-k // 64))], (k, br, wk)
        for b in range(br):
            mult = []
            for r in (r for r in rows if r["b"] == b):
                assert 0 <= r["start"] and r["start"] + 64 <= k, (k, br, wk, r)
                assert r["pos"] == b * (k + STRIDE_PAD) + r["start"], ("the loader's walk", k, br, wk, r)
                for g in r["steps"]:  # the K groups add into partial sums of their own; within the chunk their steps ascend with the group
                    for s, upper in g:
                        mult += range(r["start"] + 16 * s + (8 if upper else 0), r["start"] + 16 * s + 16)
            assert mult == list(range(k)), (k, br, wk, b)


def test_the_loaders_steps_are_64s_and_k_mod_64(walk):
    cases, _, _ = walk
    for (k, br, wk), rows in cases.items():
        pos = [r["pos"] for r in rows if r["b"] == 0]
        steps = [b - a for a, b in zip(pos, pos[1:])]
        assert steps == [64] * (len(pos) - 2) + [k % 64], (k, steps)
        assert sum(steps) + 64 == k, "the last chunk ends at k"
        assert pos[-1] % 8 == 0, "the shifted start: 16 bytes of A, whole pair-rows, VNNI-4 group rows and flat rows"
        if br > 1:  # the batch wrap: the element's stride less the last chunk's start
            nxt = [r["pos"] for r in rows if r["b"] == 1][0]
            assert nxt - pos[-1] == (k + STRIDE_PAD) - (k - 64)


def test_every_last_chunk_has_one_half_step_and_it_is_the_first_that_runs(walk):
    cases, _, _ = walk
    group_keeps = set()  # what K group 0 of the K2 tile keeps of a last chunk, in half steps
    for (k, br, wk), rows in cases.items():
        share = 4 // wk
        for r in rows:
            last = r["c"] == -(-k // 64) - 1
            assert r["skip"] == ((64 - k % 64) // 8 if last else 0), (k, r)
            assert r["skip"] in ((1, 3, 5, 7) if last else (0,))
            assert r["start"] == (k - 64 if last else 64 * r["c"]), (k, r)
            assert len(r["steps"]) == wk
            ran = [su for g in r["steps"] for su in g]
            assert [s for s, _ in ran] == list(range(r["skip"] // 2, 4)), ("the steps that run are a suffix of the chunk", k, r)
            halves = [i for i, (_, u) in enumerate(ran) if u]
            assert halves == ([0] if last else []), ("exactly one half step in a last chunk, the first step that runs", k, r)
            for g, steps in enumerate(r["steps"]):
                assert all(g * share <= s < (g + 1) * share for s, _ in steps), ("a group runs steps of its own share only", k, r)
            if last and wk == 2:
                group_keeps.add(sum(1 if u else 2 for _, u in r["steps"][0]))
    # group 0 of K2 owns steps 0 and 1: o = 56, 40 leave it nothing, o = 24 half a step, o = 8 one and a half steps
    assert group_keeps == {0, 1, 3}
