"""CPU check of the bf16 loader-wave launch table (tpp-mlir_amd/csrc/brgemm_bf16_lw_launch.h): the header the kernel, its launchers and the
planner include, compiled as plain host C++ with tests/blw_launch_table/driver.cpp. The instances blw_instance_exists names are exactly the
120 kernel symbols of the code object this table was introduced against (tests/golden/blw_instances.txt, harvested from that compile, not
written from the table), the code object of this tree holds exactly those and none uses scratch, and blw_launch_ok takes one launch per
mode and refuses one per term of each mode's rule."""
import os

import pytest

import blw_codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "blw_instances.txt")
LAYER, ITEMS, QUADS, EDGE, KEDGE, CHAIN_EDGE, KEDGE8, CHAIN_ROUNDS = range(8)
TILE = [(32, 64), (64, 64), (64, 128), (128, 128), (32, 32)]


def launch(mode, tile, b_kind, m, n, layers, chain=0, groups=0, nlayers=None):
    """a line of the driver's input; layers: [(k, br), ..]"""
    return "%d %d %d %d %d %d %d %d %s" % (mode, tile, b_kind, chain, m, n, len(layers) if nlayers is None else nlayers, groups,
                                           " ".join("%d %d" % kb for kb in layers))


@pytest.fixture(scope="module")
def table():
    return blw_codeobj.launch_table()[0]


def golden():
    with open(GOLDEN) as f:
        return f.read().split()


def test_the_table_names_exactly_the_golden_instances(table):
    want = golden()
    assert len(want) == len(set(want)) == 120
    got = [t[-1] for t in table]
    assert len(got) == len(set(got)), "a combination is listed twice"
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    # the counts of the table's rows: plain 18 + 4, edge 18, both ragged k 12 each, items 12, quads 2, chain 18, both other chains 12
    count = lambda mode, multi: sum(1 for t in table if t[0] == mode and t[1] == multi)
    assert [count(LAYER, 0), count(EDGE, 0), count(KEDGE, 0), count(KEDGE8, 0), count(ITEMS, 0), count(QUADS, 0)] == [22, 18, 12, 12, 12, 2]
    assert [count(LAYER, 1), count(CHAIN_EDGE, 1), count(CHAIN_ROUNDS, 1)] == [18, 12, 12]
    for mode, multi, tile, b_kind, sup, tup, (bm, bn), _ in table:
        assert (bm, bn) == TILE[tile] == (32 * tup[0] * tup[3], 32 * tup[1] * tup[4])
        assert len({t[5] for t in table if t[2] == tile}) == 1, "one configuration per tile"


def test_the_code_object_holds_exactly_the_golden_instances_and_no_scratch():
    rep = blw_codeobj.report()
    want = golden()
    assert sorted(rep) == sorted(want), (sorted(set(rep) - set(want)), sorted(set(want) - set(rep)))
    assert len(rep) == 120
    assert not {n: x for n, x in rep.items() if x[0]}, "an instance uses scratch"


def test_launch_ok_takes_one_launch_per_mode_and_refuses_one_per_term():
    L3 = [(192, 1), (128, 1), (128, 2)]  # three layers in whole chunks
    cases = [
        # plain layer: br >= 1, k >= 64; tiles 0 .. 4 for VNNI-2 and VNNI-4, 0 .. 3 for flat B; any k from 64 on
        (1, launch(LAYER, 1, 0, 64, 64, [(64, 1)])), (1, launch(LAYER, 4, 4, 32, 32, [(100, 3)])), (1, launch(LAYER, 3, 2, 128, 128, [(64, 1)])),
        (0, launch(LAYER, 1, 0, 64, 64, [(64, 0)])), (0, launch(LAYER, 1, 0, 64, 64, [(63, 1)])), (0, launch(LAYER, 4, 2, 32, 32, [(64, 1)])),
        (0, launch(LAYER, 5, 0, 64, 64, [(64, 1)])), (0, launch(LAYER, -1, 0, 64, 64, [(64, 1)])),
        (0, launch(LAYER, 1, 1, 64, 64, [(64, 1)])), (0, launch(LAYER, 1, 3, 64, 64, [(64, 1)])),
        # edge: tiles 0 .. 3, the three images, one layer, m >= BM, n >= BN, br >= 1, k >= 64, k % 64 == 0
        (1, launch(EDGE, 3, 2, 130, 136, [(128, 1)])), (1, launch(EDGE, 0, 0, 32, 64, [(64, 1)])),
        (0, launch(EDGE, 4, 0, 130, 136, [(128, 1)])), (0, launch(EDGE, 3, 1, 130, 136, [(128, 1)])), (0, launch(EDGE, 3, 0, 130, 136, [(128, 1)] * 2)),
        (0, launch(EDGE, 3, 0, 127, 136, [(128, 1)])), (0, launch(EDGE, 3, 0, 130, 127, [(128, 1)])), (0, launch(EDGE, 3, 0, 130, 136, [(128, 0)])),
        (0, launch(EDGE, 3, 0, 130, 136, [(32, 1)])), (0, launch(EDGE, 3, 0, 130, 136, [(1000, 1)])), (0, launch(EDGE, 3, 0, 130, 136, [(80, 1)])),
        # ragged k: as edge + n % 8 == 0, k >= 64 a multiple of 16 but not of 64
        (1, launch(KEDGE, 3, 4, 130, 136, [(80, 2)])), (1, launch(KEDGE, 2, 0, 64, 128, [(1008, 1)])),
        (0, launch(KEDGE, 3, 0, 130, 132, [(80, 1)])), (0, launch(KEDGE, 3, 0, 130, 136, [(128, 1)])), (0, launch(KEDGE, 3, 0, 130, 136, [(72, 1)])),
        (0, launch(KEDGE, 3, 0, 130, 136, [(48, 1)])), (0, launch(KEDGE, 4, 0, 130, 136, [(80, 1)])), (0, launch(KEDGE, 3, 5, 130, 136, [(80, 1)])),
        (0, launch(KEDGE, 3, 0, 130, 136, [(80, 1)] * 2)), (0, launch(KEDGE, 3, 0, 100, 136, [(80, 1)])), (0, launch(KEDGE, 3, 0, 130, 120, [(80, 1)])),
        (0, launch(KEDGE, 3, 0, 130, 136, [(80, 0)])),
        # half steps: as ragged k, k >= 64 a multiple of 8 but not of 16 - 1000, 200, 72 (72 at tile 3)
        (1, launch(KEDGE8, 3, 0, 130, 136, [(1000, 1)])), (1, launch(KEDGE8, 3, 0, 128, 128, [(72, 1)])), (1, launch(KEDGE8, 0, 2, 40, 72, [(200, 3)])),
        (0, launch(KEDGE8, 3, 0, 130, 136, [(80, 1)])), (0, launch(KEDGE8, 3, 0, 130, 136, [(128, 1)])), (0, launch(KEDGE8, 3, 0, 130, 136, [(76, 1)])),
        (0, launch(KEDGE8, 3, 0, 130, 136, [(56, 1)])), (0, launch(KEDGE8, 3, 0, 130, 132, [(72, 1)])), (0, launch(KEDGE8, 4, 0, 130, 136, [(72, 1)])),
        (0, launch(KEDGE8, 3, 3, 130, 136, [(72, 1)])), (0, launch(KEDGE8, 3, 0, 130, 136, [(72, 1)] * 2)), (0, launch(KEDGE8, 3, 0, 127, 136, [(72, 1)])),
        (0, launch(KEDGE8, 3, 0, 130, 120, [(72, 1)])), (0, launch(KEDGE8, 3, 0, 130, 136, [(72, 0)])),
        # items: k >= 64, k % 64 == 0, tiles 0, 1 and 4, VNNI-2 and VNNI-4 (an item's n may be ragged, its batch count is the item's)
        (1, launch(ITEMS, 4, 4, 64, 48, [(128, 0)])), (1, launch(ITEMS, 0, 0, 64, 64, [(64, 1)])), (1, launch(ITEMS, 1, 0, 64, 64, [(64, 1)])),
        (0, launch(ITEMS, 2, 0, 64, 128, [(64, 1)])), (0, launch(ITEMS, 3, 0, 128, 128, [(64, 1)])), (0, launch(ITEMS, 1, 2, 64, 64, [(64, 1)])),
        (0, launch(ITEMS, 1, 0, 64, 64, [(32, 1)])), (0, launch(ITEMS, 1, 0, 64, 64, [(96, 1)])),
        # quads: k >= 64, k % 64 == 0, m == n == 128, VNNI-2 and VNNI-4
        (1, launch(QUADS, 3, 0, 128, 128, [(64, 1)])), (1, launch(QUADS, 3, 4, 128, 128, [(1024, 4)])),
        (0, launch(QUADS, 3, 2, 128, 128, [(64, 1)])), (0, launch(QUADS, 3, 0, 64, 128, [(64, 1)])), (0, launch(QUADS, 3, 0, 128, 256, [(64, 1)])),
        (0, launch(QUADS, 3, 0, 128, 128, [(32, 1)])), (0, launch(QUADS, 3, 0, 128, 128, [(80, 1)])),
        # chain: tiles 0 .. 3 (and, the one tightening, a B image that is none of the three)
        (1, launch(LAYER, 3, 2, 256, 256, L3, chain=1)), (1, launch(LAYER, 0, 0, 64, 64, L3, chain=1)),
        (0, launch(LAYER, 4, 0, 64, 64, L3, chain=1)), (0, launch(LAYER, -1, 0, 64, 64, L3, chain=1)), (0, launch(LAYER, 1, 1, 64, 64, L3, chain=1)),
        # ragged chain: tiles 0 .. 3, the three images, 2 <= L <= 8, m >= BM, n >= BN, n % BN == 0; every layer br >= 1, k >= 64, k % 64 == 0
        (1, launch(CHAIN_EDGE, 1, 0, 1000, 1024, L3, chain=1)), (1, launch(CHAIN_EDGE, 3, 4, 130, 128, [(64, 1)] * 8, chain=1)),
        (1, launch(CHAIN_EDGE, 0, 2, 40, 64, [(64, 1)] * 2, chain=1)),
        (0, launch(CHAIN_EDGE, 1, 0, 1000, 1032, L3, chain=1)), (0, launch(CHAIN_EDGE, 4, 0, 1000, 1024, L3, chain=1)),
        (0, launch(CHAIN_EDGE, 1, 3, 1000, 1024, L3, chain=1)), (0, launch(CHAIN_EDGE, 1, 0, 1000, 1024, [(64, 1)], chain=1)),
        (0, launch(CHAIN_EDGE, 1, 0, 1000, 1024, [(64, 1)] * 8, chain=1, nlayers=9)), (0, launch(CHAIN_EDGE, 1, 0, 60, 1024, L3, chain=1)),
        (0, launch(CHAIN_EDGE, 2, 0, 1000, 64, L3, chain=1)), (0, launch(CHAIN_EDGE, 1, 0, 1000, 1024, [(192, 1), (128, 0), (128, 1)], chain=1)),
        (0, launch(CHAIN_EDGE, 1, 0, 1000, 1024, [(192, 1), (128, 1), (32, 1)], chain=1)),
        (0, launch(CHAIN_EDGE, 1, 0, 1000, 1024, [(192, 1), (200, 1), (128, 1)], chain=1)),
        # multi-round chain: as a ragged chain + m % BM == 0 and 1 <= groups <= m / BM
        (1, launch(CHAIN_ROUNDS, 3, 0, 640, 256, L3, chain=1, groups=2)), (1, launch(CHAIN_ROUNDS, 3, 0, 640, 256, L3, chain=1, groups=5)),
        (1, launch(CHAIN_ROUNDS, 0, 4, 96, 64, [(64, 1)] * 8, chain=1, groups=1)),
        (0, launch(CHAIN_ROUNDS, 3, 0, 640, 256, L3, chain=1, groups=0)), (0, launch(CHAIN_ROUNDS, 3, 0, 640, 256, L3, chain=1, groups=6)),
        (0, launch(CHAIN_ROUNDS, 3, 0, 650, 256, L3, chain=1, groups=2)), (0, launch(CHAIN_ROUNDS, 3, 0, 640, 264, L3, chain=1, groups=2)),
        (0, launch(CHAIN_ROUNDS, 4, 0, 640, 256, L3, chain=1, groups=2)), (0, launch(CHAIN_ROUNDS, 3, 1, 640, 256, L3, chain=1, groups=2)),
        (0, launch(CHAIN_ROUNDS, 3, 0, 640, 256, [(64, 1)], chain=1, groups=2)),
        (0, launch(CHAIN_ROUNDS, 3, 0, 640, 256, [(64, 1)] * 8, chain=1, groups=2, nlayers=9)),
        (0, launch(CHAIN_ROUNDS, 3, 0, 64, 256, L3, chain=1, groups=1)), (0, launch(CHAIN_ROUNDS, 3, 0, 640, 64, L3, chain=1, groups=2)),
        (0, launch(CHAIN_ROUNDS, 3, 0, 640, 256, [(192, 0), (128, 1), (128, 1)], chain=1, groups=2)),
        (0, launch(CHAIN_ROUNDS, 3, 0, 640, 256, [(192, 1), (128, 1), (1000, 1)], chain=1, groups=2)),
        (0, launch(CHAIN_ROUNDS, 3, 0, 640, 256, [(32, 1), (128, 1), (128, 1)], chain=1, groups=2)),
        # no such mode
        (0, launch(8, 1, 0, 64, 64, [(64, 1)])), (0, launch(-1, 1, 0, 64, 64, [(64, 1)])),
    ]
    _, ok = blw_codeobj.launch_table([c[1] for c in cases])
    wrong = [(want, line, got) for (want, line), got in zip(cases, ok) if want != got]
    assert not wrong, wrong
    assert {int(c[1].split()[0]) for c in cases if c[0]} == set(range(8)), "an accepting case per mode"
