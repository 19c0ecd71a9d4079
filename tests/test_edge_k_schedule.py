"""CPU check of the ragged-k schedule (tpp-mlir_amd/csrc/brgemm_f32_lw_kedge.h, xsmm_hip_set_edge_k): the header the kernel, its launcher
and the planner include, compiled as plain host C++ with tests/edge_k_schedule/driver.cpp. For every k in 64 .. 640 in steps of 8 that is
no multiple of 64, 1 .. 3 batch elements and K splits 1, 2, 4: the k-values multiplied are exactly 0 .. k - 1 of each batch element, each
once, in ascending order; no chunk starts below 0 or ends beyond k; the loader's walk lands on every chunk's start; what a K group keeps
of its share is a suffix of it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

KS = [k for k in range(64, 641, 8) if k % 64]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("edge_k_schedule") / "schedule")
    subprocess.check_call([cc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "edge_k_schedule", "driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    cases, ok = {}, {}
    for l in out:
        f = l.split()
        if f[0] == "ok":
            ok[int(f[1])] = int(f[2])
            continue
        k, br, wk, b, c = (int(x) for x in f[:5])
        cases.setdefault((k, br, wk), []).append(dict(b=b, c=c, pos=int(f[5][1:]), start=int(f[6][1:]), skip=int(f[7][1:]),
                                                      kept=[[int(d) for d in g] for g in f[8].split(",")] if len(f) > 8 else [[]]))
    return cases, ok


def test_every_case_is_there(walk):
    cases, ok = walk
    assert sorted(cases) == [(k, br, wk) for k in KS for br in (1, 2, 3) for wk in (1, 2, 4)]
    assert len(KS) == 63
    assert ok == {0: 0, 8: 0, 56: 0, 64: 0, 100: 0, 128: 0, 132: 0, 636: 0, 640: 0}  # none of these is taken
    assert all(k >= 64 and k % 8 == 0 and k % 64 for k in KS)


def test_the_k_values_multiplied_are_each_batch_element_once_in_order(walk):
    cases, _ = walk
    for (k, br, wk), rows in cases.items():
        assert [(r["b"], r["c"]) for r in rows] == [(b, c) for b in range(br) for c in range(-(-k // 64))], (k, br, wk)
        for b in range(br):
            mult = []
            for r in (r for r in rows if r["b"] == b):
                assert 0 <= r["start"] and r["start"] + 64 <= k, (k, br, wk, r)
                assert r["pos"] == b * (k + 24) + r["start"], ("the loader's walk", k, br, wk, r)
                for g in r["kept"]:  # the K groups add into partial sums of their own; within the chunk their blocks ascend with the group
                    for kb in g:
                        mult += range(r["start"] + 8 * kb, r["start"] + 8 * kb + 8)
            assert mult == list(range(k)), (k, br, wk, b)


def test_only_the_last_chunk_skips_and_a_group_keeps_a_suffix_of_its_share(walk):
    cases, _ = walk
    seen_whole_group_skipped = set()
    for (k, br, wk), rows in cases.items():
        share = 8 // wk
        for r in rows:
            last = r["c"] == -(-k // 64) - 1
            assert r["skip"] == ((64 - k % 64) // 8 if last else 0), (k, r)
            assert r["start"] == (k - 64 if last else 64 * r["c"]), (k, r)
            assert len(r["kept"]) == wk
            for g, kept in enumerate(r["kept"]):
                own = list(range(g * share, (g + 1) * share))
                assert kept == own[len(own) - len(kept):], ("not a suffix of the group's share", k, wk, g, r)
                assert kept == [kb for kb in own if kb >= r["skip"]]
                if last and not kept:
                    seen_whole_group_skipped.add(wk)
    assert seen_whole_group_skipped == {2, 4}, "k = 96 skips the whole share of group 0 of K2 and K4"
