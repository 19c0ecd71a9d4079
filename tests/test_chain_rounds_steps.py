"""CPU check of the step maps of a multi-round layer chain (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_rounds.h, xsmm_hip_set_chain_rounds): the
header the chain kernel on G resident row groups, its launcher and the planner include, compiled as plain host C++ with
tests/chain_rounds_steps/driver.cpp. The maps do not depend on the tile's shape - they count row blocks - so one walk stands for all four
tiles; the rule's groups are checked for the tile grids of each. For every tiles_m in 1 .. 40 and every G in 1 .. tiles_m, three layers:
every (layer, row block) is computed by exactly one group, exactly once; a simulation of the groups' step sequences with the counters
completes under round-robin, reverse and seeded-random scheduling of the groups; every wait names the counter of the block whose rows the
step loads, in the layer before; and the steps go layer-major, the order the progress argument of the kernel rests on."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

L = 3
TILES = ((32, 64), (64, 64), (64, 128), (128, 128))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("chain_rounds_steps") / "steps")
    # C++14: the header is for any host compiler of that standard
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "chain_rounds_steps", "driver.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()


@pytest.fixture(scope="module")
def walks(out):
    """(tiles_m, G) -> per group: (steps per layer, rounds, [(layer, block, wait layer, wait block)])"""
    cases = {}
    for line in out:
        if line.startswith("rule"):
            continue
        head, steps = line.split(" :")
        f = head.split()
        tiles_m, G, g = int(f[0]), int(f[1]), int(f[2])
        seq = [tuple(int(x) for x in s.split(".")) for s in steps.split()]
        cases.setdefault((tiles_m, G), {})[g] = (int(f[3][1:]), int(f[4][1:]), seq)
    return cases


def test_every_case_is_there(walks):
    assert sorted(walks) == [(t, G) for t in range(1, 41) for G in range(1, t + 1)]
    for (tiles_m, G), groups in walks.items():
        assert sorted(groups) == list(range(G)), (tiles_m, G)


def test_every_layer_and_row_block_is_computed_by_exactly_one_group_exactly_once(walks):
    for (tiles_m, G), groups in walks.items():
        seen = {}
        for g, (n, R, seq) in groups.items():
            assert R == -(-tiles_m // G) and n == len([b for b in range(tiles_m) if b % G == g]), (tiles_m, G, g)
            assert len(seq) == L * n and 1 <= n <= R, (tiles_m, G, g)
            for (l, tm, _, _) in seq:
                assert 0 <= l < L and 0 <= tm < tiles_m and tm % G == g, ("a block of another group, or outside the matrix", tiles_m, G, g, l, tm)
                assert (l, tm) not in seen, ("computed twice", tiles_m, G, l, tm, g, seen[(l, tm)])
                seen[(l, tm)] = g
        assert sorted(seen) == [(l, tm) for l in range(L) for tm in range(tiles_m)], (tiles_m, G)
        assert max(n for n, _, _ in groups.values()) == -(-tiles_m // G), "group 0 walks every round"


def test_the_steps_go_layer_major_and_rounds_ascend(walks):
    for (tiles_m, G), groups in walks.items():
        for g, (n, _, seq) in groups.items():
            assert [(l, tm) for (l, tm, _, _) in seq] == [(l, g + r * G) for l in range(L) for r in range(n)], (tiles_m, G, g)


def test_every_wait_names_the_counter_of_the_block_whose_rows_the_step_loads(walks):
    for (tiles_m, G), groups in walks.items():
        for g, (_, _, seq) in groups.items():
            for (l, tm, wl, wtm) in seq:
                # the step loads rows [tm * BM, (tm + 1) * BM) of layer l - 1's output: stored by row block tm of that layer, no other
                assert (wl, wtm) == ((l - 1, tm) if l > 0 else (-1, -1)), (tiles_m, G, g, l, tm, wl, wtm)


def simulate(groups, tiles_n, order, burst=1):
    """G x tiles_n workgroups, each at a position of its group's step sequence; a workgroup may make its next step when the counter its
    step waits for has all tiles_n arrivals; making a step of layer l < L - 1 adds one arrival to cnt[l][tm]. `order` yields the
    workgroup to try next, every workgroup at least once in any 2 * burst * (number of workgroups) turns. True when every workgroup has
    finished and every counter has exactly tiles_n arrivals; False when nobody could move for that many turns."""
    cnt = {}
    wgs = [(g, tn) for g in sorted(groups) for tn in range(tiles_n)]
    pos = {w: 0 for w in wgs}
    left = sum(len(groups[g][2]) for g, _ in wgs)
    stuck = 0
    for w in order(wgs):
        seq = groups[w[0]][2]
        if pos[w] == len(seq):
            stuck += 1
        else:
            l, tm, wl, wtm = seq[pos[w]]
            if wl >= 0 and cnt.get((wl, wtm), 0) < tiles_n:
                stuck += 1
            else:
                if l < L - 1:
                    cnt[(l, tm)] = cnt.get((l, tm), 0) + 1
                pos[w] += 1
                left -= 1
                stuck = 0
        if left == 0:
            return all(v == tiles_n for v in cnt.values())
        if stuck > 2 * burst * len(wgs):
            return False
    return False


def round_robin(wgs):
    while True:
        for w in wgs:
            yield w


def reverse(wgs):
    while True:
        for w in reversed(wgs):
            yield w


def seeded(seed):
    def order(wgs):
        rng = random.Random(seed)
        while True:
            sweep = list(wgs)
            rng.shuffle(sweep)
            for w in sweep:
                yield w
    return order


BURST = 4 * L * 16  # more turns than any workgroup of the cases below has steps


def greedy_last_first(wgs):
    """every workgroup runs as far as it can before the next one gets a turn, the last workgroup first"""
    while True:
        for w in reversed(wgs):
            for _ in range(BURST):
                yield w


@pytest.mark.parametrize("name,order", [("round_robin", round_robin), ("reverse", reverse), ("random_1", seeded(1)), ("random_2", seeded(2))])
def test_the_counters_let_every_schedule_complete(walks, name, order):
    for (tiles_m, G), groups in walks.items():
        for tiles_n in ((1, 2) if tiles_m > 12 else (1, 2, 3)):
            assert simulate(groups, tiles_n, order), (name, tiles_m, G, tiles_n)


def test_a_schedule_that_runs_one_workgroup_at_a_time_completes_too(walks):
    for (tiles_m, G), groups in walks.items():
        if tiles_m <= 16:
            assert simulate(groups, 2, greedy_last_first, BURST), (tiles_m, G)


def test_the_simulation_notices_a_cyclic_wait(walks):
    """the check has teeth: were a step of layer 1 to wait for ITS OWN layer's counter of the next row block - a step that is not earlier in
    anybody's order - the waits would form a cycle over the row blocks, and no schedule completes"""
    groups = {g: (n, R, [(l, tm, l, (tm + 1) % 5) if l == 1 else (l, tm, wl, wtm) for (l, tm, wl, wtm) in seq]) for g, (n, R, seq) in walks[(5, 2)].items()}
    for order, burst in ((round_robin, 1), (greedy_last_first, BURST)):
        assert not simulate(groups, 1, order, burst)


def test_groups_and_rounds_of_the_rule(out):
    seen = 0
    for line in out:
        if not line.startswith("rule"):
            continue
        f = line.split()
        tiles_m, tiles_n, cus = int(f[1]), int(f[2]), int(f[3])
        gmax, G, R = int(f[4][4:]), int(f[5][1:]), int(f[6][1:])
        assert gmax == cus // tiles_n, line
        if gmax == 0:
            assert (G, R) == (0, 0), line
            continue
        seen += 1
        want_r = -(-tiles_m // gmax)
        assert R == want_r and G == -(-tiles_m // want_r) and 1 <= G <= gmax and G * tiles_n <= cus, line
        assert -(-tiles_m // G) == R, ("balancing the rounds may not add one", line)
    assert seen > 500
    # the issue's examples, on the 128x128 tile of three 1024-wide layers at 256 compute units
    bm, bn = TILES[3]
    for rows, g, r in ((8192, 32, 2), (4224, 17, 2), (32768, 32, 8)):
        line = [l for l in out if l.startswith("rule %d %d 256 " % (rows // bm, 1024 // bn))]
        assert line and line[0].split()[5:] == ["G%d" % g, "R%d" % r], (rows, line)
