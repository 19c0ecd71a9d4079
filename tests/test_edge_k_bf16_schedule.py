"""CPU check of the bf16 ragged-k schedule (tpp-mlir_amd/csrc/brgemm_bf16_lw_kedge.h, xsmm_hip_set_edge_k_bf16): the header the kernel, its
launcher and the planner include, compiled as plain host C++ with tests/edge_k_bf16_schedule/driver.cpp. For every k in 64 .. 640 in steps
of 16 that is no multiple of 64, 1 .. 3 batch elements and K splits 1 and 2: the k-values multiplied are exactly 0 .. k - 1 of each batch
element, each once, in ascending order; no chunk starts below 0 or ends beyond k; the loader's steps land on every chunk's start and sum
to the element's length; what a K group keeps of its share of a last chunk is a suffix of it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

KS = [k for k in range(64, 641, 16) if k % 64]
STRIDE_PAD = 40  # the driver's batch stride is k + 40


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("edge_k_bf16_schedule") / "schedule")
    # C++14: the header is for any host compiler of that standard
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "edge_k_bf16_schedule", "driver.cpp"), "-o", exe])
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
        cases.setdefault((k, br, wk), []).append(dict(b=b, c=c, pos=int(f[5][1:]), start=int(f[6][1:]), skip=int(f[7][1:]),
                                                      kept=[[int(d) for d in g] for g in f[8].split(",")] if len(f) > 8 else [[]]))
    return cases, ok, facts


def test_every_case_is_there(walk):
    cases, ok, facts = walk
    assert sorted(cases) == [(k, br, wk) for k in KS for br in (1, 2, 3) for wk in (1, 2)]
    assert len(KS) == 27 and all(k >= 64 and k % 16 == 0 and k % 64 for k in KS)
    # none of these is taken: below a chunk, whole chunks, k % 16 != 0
    assert ok == {0: 0, 16: 0, 48: 0, 64: 0, 72: 0, 100: 0, 128: 0, 136: 0, 200: 0, 632: 0, 640: 0, 1000: 0}
    # (chunks per element, o, skipped steps) of the lengths the GPU tests and the A/B run
    assert facts == {80: (2, 48, 3), 96: (2, 32, 2), 112: (2, 16, 1), 160: (3, 32, 2), 272: (5, 48, 3), 560: (9, 16, 1), 784: (13, 48, 3)}


def test_the_k_values_multiplied_are_each_batch_element_once_in_order(walk):
    cases, _, _ = walk
    for (k, br, wk), rows in cases.items():
        assert [(r["b"], r["c"]) for r in rows] == [(b, c) for b in range(br) for c in range(-(-k // 64))], (k, br, wk)
        for b in range(br):
            mult = []
            for r in (r for r in rows if r["b"] == b):
                assert 0 <= r["start"] and r["start"] + 64 <= k, (k, br, wk, r)
                assert r["pos"] == b * (k + STRIDE_PAD) + r["start"], ("the loader's walk", k, br, wk, r)
                for g in r["kept"]:  # the K groups add into partial sums of their own; within the chunk their steps ascend with the group
                    for s in g:
                        mult += range(r["start"] + 16 * s, r["start"] + 16 * s + 16)
            assert mult == list(range(k)), (k, br, wk, b)


def test_the_loaders_steps_sum_to_the_elements_length(walk):
    cases, _, _ = walk
    for (k, br, wk), rows in cases.items():
        pos = [r["pos"] for r in rows if r["b"] == 0]
        steps = [b - a for a, b in zip(pos, pos[1:])]
        assert steps == [64] * (len(pos) - 2) + [k % 64], (k, steps)
        assert sum(steps) + 64 == k, "the last chunk ends at k"
        assert (pos[-1] * 2) % 16 == 0 and pos[-1] % 4 == 0, "the shifted start: 16 bytes of A, whole pair-rows and VNNI-4 group rows"
        if br > 1:  # the batch wrap: the element's stride less the last chunk's start
            nxt = [r["pos"] for r in rows if r["b"] == 1][0]
            assert nxt - pos[-1] == (k + STRIDE_PAD) - (k - 64)


def test_only_the_last_chunk_skips_and_a_group_keeps_a_suffix_of_its_share(walk):
    cases, _, _ = walk
    seen_whole_group_skipped = set()
    for (k, br, wk), rows in cases.items():
        share = 4 // wk
        for r in rows:
            last = r["c"] == -(-k // 64) - 1
            assert r["skip"] == ((64 - k % 64) // 16 if last else 0), (k, r)
            assert r["skip"] in ((1, 2, 3) if last else (0,))
            assert r["start"] == (k - 64 if last else 64 * r["c"]), (k, r)
            assert len(r["kept"]) == wk
            for g, kept in enumerate(r["kept"]):
                own = list(range(g * share, (g + 1) * share))
                assert kept == own[len(own) - len(kept):], ("not a suffix of the group's share", k, wk, g, r)
                assert kept == [s for s in own if s >= r["skip"]]
                if last and not kept:
                    seen_whole_group_skipped.add((wk, g))
    assert seen_whole_group_skipped == {(2, 0)}, "k % 64 = 32 or 16 skips the whole share of group 0 of K2; some step of a chunk always runs"
