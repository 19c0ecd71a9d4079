"""CPU check of the per-layer schedule of a ragged-width layer chain (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_ragged.h, xsmm_hip_set_chain_ragged):
the header the chain kernel's loader and K loop, its launcher and the planner include, compiled as plain host C++ with
tests/chain_ragged_schedule/driver.cpp. Ring depths 4, 6 and 8; chains of 2 .. 4 layers with k from {64, 72, 80, 88, 96, 104, 112, 120, 128,
200, 784, 1000} and 1 .. 3 batch elements. Every k-value of every batch element is multiplied exactly once, counted in halves of a k-step;
no chunk leaves [0, k); the skipped halves take every value 0 .. 7; the loader's and the K loop's slot sequences agree chunk for chunk across
layer boundaries, with each other and with the header's slot function; and every layer's first slot follows from the layers before it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

KS = [64, 72, 80, 88, 96, 104, 112, 120, 128, 200, 784, 1000]
NONE, UPPER, WHOLE = 0, 1, 2


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("chain_ragged_schedule") / "schedule")
    # C++14: the header is for any host compiler of that standard
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "chain_ragged_schedule", "driver.cpp"), "-o", exe])
    out, cur = [], None
    for line in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = line.split()
        if f[0] == "chain":
            cur = dict(nslot=int(f[1]), layers=[tuple(int(x) for x in kb.split(":")) for kb in f[3:]], chunks=[])
            assert len(cur["layers"]) == int(f[2])
            out.append(cur)
        else:
            cur["chunks"].append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), [int(c) for c in f[5]]) + tuple(int(x) for x in f[6:]))
    return out


def test_the_case_list_is_the_issue_s(cases):
    assert {c["nslot"] for c in cases} == {4, 6, 8}
    assert {len(c["layers"]) for c in cases} == {2, 3, 4}
    assert {k for c in cases for k, _ in c["layers"]} == set(KS) and {b for c in cases for _, b in c["layers"]} == {1, 2, 3}
    for nslot in (4, 6, 8):
        assert {tuple(c["layers"]) for c in cases if c["nslot"] == nslot and len(c["layers"]) == 2} == {((a, x), (b, y)) for a in KS for b in KS for x in (1, 2, 3) for y in (1, 2, 3)}


def test_every_k_value_is_multiplied_exactly_once_and_no_chunk_leaves_the_element(cases):
    skips = set()
    for c in cases:
        for l, (k, br) in enumerate(c["layers"]):
            halves = [[0] * (k // 8) for _ in range(br)]
            mine = [x for x in c["chunks"] if x[0] == l]
            assert [x[1] for x in mine] == list(range(br * -(-k // 64))), (c["layers"], l)
            for (_, idx, batch, k0, skip, parts, *_rest) in mine:
                assert 0 <= k0 and k0 + 64 <= k and k0 % 8 == 0, (k, idx, k0)
                assert batch == idx // -(-k // 64)
                skips.add(skip)
                for s, part in enumerate(parts):  # k-step s: k-values k0 + 16 s .. + 15, the lower and the upper half
                    lo, hi = (k0 + 16 * s) // 8, (k0 + 16 * s) // 8 + 1
                    if part == WHOLE:
                        halves[batch][lo] += 1
                    if part in (WHOLE, UPPER):
                        halves[batch][hi] += 1
                # the parts are the skip's: `skip` halves at the head of the chunk are not multiplied
                assert [NONE if 2 * s + 2 <= skip else UPPER if 2 * s + 1 == skip else WHOLE for s in range(4)] == parts
            assert all(h == 1 for b in halves for h in b), (c["layers"], l)
    assert skips == set(range(8)), skips


def test_a_whole_k_layer_multiplies_what_the_plain_chain_multiplies(cases):
    for c in cases:
        for l, (k, br) in enumerate(c["layers"]):
            if k % 64 == 0:
                for (_, idx, batch, k0, skip, parts, *_rest) in (x for x in c["chunks"] if x[0] == l):
                    assert skip == 0 and parts == [WHOLE] * 4 and k0 == 64 * (idx % (k // 64))


def test_the_loader_and_the_k_loop_walk_the_same_slots_first_ks_and_skips(cases):
    for c in cases:
        nslot, s0, t = c["nslot"], 0, 0
        for l, (k, br) in enumerate(c["layers"]):
            mine = [x for x in c["chunks"] if x[0] == l]
            # every layer's first slot follows from the layers before it: the chunks so far, modulo the ring
            assert mine[0][6] == s0 == t % nslot, (c["layers"], l)
            for (_, idx, batch, k0, skip, parts, slot, slot_loader, k0_loader, slot_mfma, skip_mfma) in mine:
                assert slot == slot_loader == slot_mfma == (t + idx) % nslot, (c["layers"], l, idx)
                assert k0_loader == k0 and skip_mfma == skip, (c["layers"], l, idx)
            t += len(mine)
            s0 = t % nslot
    starts = {(c["nslot"], [x for x in c["chunks"] if x[0] == l][0][6]) for c in cases for l in range(1, len(c["layers"]))}
    assert starts == {(n, s) for n in (4, 6, 8) for s in range(n)}, "a later layer starts at every slot of every ring"
