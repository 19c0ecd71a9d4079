"""CPU check of the row-block arithmetic of a ragged-m layer chain (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_edge.h, xsmm_hip_set_chain_edge):
the header the chain kernel on edge row tiles, its launcher and the planner include, compiled as plain host C++ with
tests/chain_edge_blocks/driver.cpp. For every BM in {32, 64, 128} and every m in [BM, 4 BM + 7]: a divisible m gives every row block one
producer block, itself; a ragged m gives the last block the two blocks {tiles_m - 2, tiles_m - 1} and every other block itself; the rows
the blocks store cover [0, m) exactly once; no block loads or stores outside [0, m); and the blocks a block waits for are exactly the
blocks that store a row it loads - the property the two-counter wait of the kernel rests on."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

BMS = (32, 64, 128)


@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("chain_edge_blocks") / "blocks")
    # C++14: the header is for any host compiler of that standard
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "chain_edge_blocks", "driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    cases = {}
    for l in out:
        f = l.split()
        bm, m, tiles_m, tm = (int(x) for x in f[:4])
        sb, se = (int(x) for x in f[6][1:].split(":"))
        wf, wl = (int(x) for x in f[7][1:].split(":"))
        cases.setdefault((bm, m), []).append(dict(tiles_m=tiles_m, tm=tm, row0=int(f[4][1:]), own=int(f[5][1:]), sb=sb, se=se, wf=wf, wl=wl))
    return cases


def test_every_case_is_there(blocks):
    assert sorted(blocks) == [(bm, m) for bm in BMS for m in range(bm, 4 * bm + 8)]
    for (bm, m), rows in blocks.items():
        assert [r["tm"] for r in rows] == list(range(-(-m // bm))) and {r["tiles_m"] for r in rows} == {-(-m // bm)}, (bm, m)


def test_a_divisible_m_gives_every_block_one_producer_block(blocks):
    seen = 0
    for (bm, m), rows in blocks.items():
        if m % bm:
            continue
        seen += 1
        for r in rows:
            assert (r["wf"], r["wl"]) == (r["tm"], r["tm"]) and r["row0"] == r["tm"] * bm and r["own"] == 0, (bm, m, r)
    assert seen == 12


def test_a_ragged_m_gives_the_last_block_two_producer_blocks(blocks):
    for (bm, m), rows in blocks.items():
        if m % bm == 0:
            continue
        t = len(rows)
        assert t >= 2
        for r in rows[:-1]:
            assert (r["wf"], r["wl"]) == (r["tm"], r["tm"]) and r["row0"] == r["tm"] * bm and r["own"] == 0, (bm, m, r)
        last = rows[-1]
        assert (last["wf"], last["wl"]) == (t - 2, t - 1), (bm, m, last)
        assert last["row0"] == m - bm and last["own"] == t * bm - m and 0 < last["own"] < bm, (bm, m, last)


def test_own_rows_cover_every_row_exactly_once_and_nothing_leaves_the_matrix(blocks):
    for (bm, m), rows in blocks.items():
        stored = []
        for r in rows:
            assert 0 <= r["row0"] and r["row0"] + bm <= m, ("a block loads outside [0, m)", bm, m, r)
            assert r["sb"] == r["row0"] + r["own"], ("the store predicate and the owned rows disagree", bm, m, r)
            assert r["row0"] <= r["sb"] < r["se"] <= r["row0"] + bm, ("a block stores rows it did not compute", bm, m, r)
            stored += range(r["sb"], r["se"])
        assert stored == list(range(m)), (bm, m)


def test_a_block_waits_for_exactly_the_blocks_that_store_its_rows(blocks):
    for (bm, m), rows in blocks.items():
        owner = {}
        for r in rows:
            for row in range(r["sb"], r["se"]):
                owner[row] = r["tm"]
        for r in rows:
            producers = {owner[row] for row in range(r["row0"], r["row0"] + bm)}
            assert producers == set(range(r["wf"], r["wl"] + 1)), (bm, m, r, producers)
