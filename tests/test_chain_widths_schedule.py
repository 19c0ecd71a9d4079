"""CPU check of the schedule of a mixed-width layer chain (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_widths.h, xsmm_hip_set_chain_widths): the header
the chain kernel's loader and MFMA waves and its launcher include, compiled as plain host C++ with tests/chain_widths_schedule/driver.cpp. For
every tile 0 .. 3 and the width vectors (in column tiles) widen-narrow [1, 4, 1], narrow-first [1, 2, 4], funnel [8, 4, 2, 1], eight
alternating layers [2, 1] * 4, all-equal [2, 2, 2] as the degenerate case, and [3, 1, 2], [1, 3, 1], [3, 1, 3], [1, 3, 3], [4, 1], [4, 2, 4]: the driver
walks every workgroup's loader role and MFMA role. Both roles visit the same layers and execute the same barrier sequence; ring-slot
counts agree; every counter cnt[l][tm] receives exactly n_l / BN arrivals per launch; every wait is on a counter of an earlier layer and
the launch makes progress when the workgroups run in an order that blocks at waits; no workgroup is without an active layer; targets stay
correct over several epochs, also for two chains that alternate on one key - and differ for two chains of one grid with different inner
widths, which is why the counter block is keyed on every layer's column tiles."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

VECTORS = [[1, 4, 1], [1, 2, 4], [8, 4, 2, 1], [2, 1] * 4, [2, 2, 2], [3, 1, 2], [1, 3, 1], [3, 1, 3], [1, 3, 3], [4, 1], [4, 2, 4]]
BARRIERS = ("S2", "P", "m", "R1", "S1")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("chain_widths_schedule") / "schedule")
    subprocess.check_call([cc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "chain_widths_schedule", "driver.cpp"), "-o", exe])
    out, cur = [], None
    for line in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = line.split()
        if f[0] == "case":
            tile, nslot, wk, nla, L = (int(x) for x in f[1:6])
            cur = dict(tile=tile, nslot=nslot, wk=wk, nla=nla, L=L, tiles=[int(x) for x in f[6:6 + L]], chunks=[int(x) for x in f[6 + L:6 + 2 * L]], wgs=[], targets={})
            out.append(cur)
        elif f[0] == "wg":
            cur["wgs"].append(dict(tn=int(f[1]), first=int(f[3]), last=int(f[5])))
        elif f[0] in ("L", "M"):
            cur["wgs"][-1][f[0]] = f[1:]
        elif f[0] == "target":
            cur["targets"][(int(f[1]), int(f[2]))] = int(f[3])
        elif f[0] == "ok":
            LAUNCH_OK[f[1]] = int(f[2])
        elif f[0] == "inst":
            LAUNCH_OK["inst"] = [tuple(int(x) for x in i.split(":")) for i in f[1:]]
        elif f[0] == "table":
            LAUNCH_OK["table"] = [int(x) for x in f[1:]]
    return out


LAUNCH_OK = {}  # the driver's answers of blw_chain_widths_launch_ok / _instance_exists (filled by the fixture above)


def test_the_launcher_s_refusals_one_accepted_launch_and_one_refusal_per_term(cases):
    terms = ["tile-4", "b-kind-1", "one-layer", "nine-layers", "empty-batch", "k-below-64", "k-not-in-chunks", "n-below-bn", "n-not-in-tiles", "equal-widths", "m-below-bm",
             "m-not-in-blocks", "n-not-in-tiles-of-128"]
    assert LAUNCH_OK["accepted"] == 1 and {t: LAUNCH_OK[t] for t in terms} == {t: 0 for t in terms}
    assert sorted(LAUNCH_OK["inst"]) == sorted((t, b, s) for t in range(4) for b in (0, 2, 4) for s in (1, 2) if s == 1 or t < 2) and len(LAUNCH_OK["inst"]) == 18
    assert LAUNCH_OK["table"] == [8, 9, 0, 0], "BLW_MODES stays 8; the launch table goes on refusing mode 9"


def barriers(events):
    return [e for e in events if e.split(":")[0] in BARRIERS]


def layers_of(events):
    return [int(e[1:].split(":")[0]) for e in events if e[0] == "s"]


def test_the_case_list_is_the_issue_s(cases):
    assert len(cases) == 4 * len(VECTORS)
    for t in range(4):
        assert [c["tiles"] for c in cases if c["tile"] == t] == VECTORS
    assert {c["wk"] for c in cases} == {1, 2}, "tiles with and without the K-split barrier R1"


def test_no_workgroup_is_without_an_active_layer_and_first_next_last_agree_with_active(cases):
    for c in cases:
        assert [w["tn"] for w in c["wgs"]] == list(range(max(c["tiles"])))
        for w in c["wgs"]:
            active = [l for l in range(c["L"]) if w["tn"] < c["tiles"][l]]
            assert active and w["first"] == active[0] and w["last"] == active[-1]
            assert layers_of(w["L"]) == layers_of(w["M"]) == active, (c["tiles"], w["tn"])


def test_both_roles_execute_the_same_barriers_and_count_the_same_ring_slots(cases):
    for c in cases:
        for w in c["wgs"]:
            bm = barriers(w["M"])
            if c["wk"] > 1 and bm[-1] == "R1:%d" % (c["L"] - 1):
                bm = bm[:-1]  # (the chain's last layer: the loaders have ended in front of its R1 - ended waves take no part in barriers)
            assert barriers(w["L"]) == bm, (c["tile"], c["tiles"], w["tn"])
            assert [e for e in w["L"] if e[0] == "s"] == [e for e in w["M"] if e[0] == "s"]
            s0 = 0
            for l in layers_of(w["M"]):  # s0 advances by T on active layers only
                assert "s%d:%d" % (l, s0) in w["M"]
                s0 = (s0 + c["chunks"][l]) % c["nslot"]
            # per active layer: P, one barrier per further chunk, R1 on a K-split tile, and S1 after every layer but the chain's last
            for l in layers_of(w["M"]):
                b = [e for e in barriers(w["M"]) if e.endswith(":%d" % l)]
                want = (["S2:%d" % l] if c["nla"] > 1 and l > 0 else []) + ["P:%d" % l] + ["m:%d" % l] * (c["chunks"][l] - 1)
                want += (["R1:%d" % l] if c["wk"] > 1 else []) + (["S1:%d" % l] if l + 1 < c["L"] else [])
                assert b == want, (c["tiles"], w["tn"], l)


def test_a_non_final_last_active_layer_runs_the_whole_seam(cases):
    seen = 0
    for c in cases:
        for w in c["wgs"]:
            if w["last"] + 1 < c["L"]:
                seen += 1
                assert w["M"][-2:] == ["S1:%d" % w["last"], "A%d" % w["last"]] and w["L"][-1] == "S1:%d" % w["last"]
            else:
                assert not any(e == "A%d" % w["last"] for e in w["M"]), "the chain's last layer goes unsignalled"
    assert seen


def test_the_run_ahead_targets_the_next_active_layer(cases):
    seen = 0
    for c in cases:
        for w in c["wgs"]:
            act = layers_of(w["L"])
            for e in (e for e in w["L"] if e[0] == "I"):
                l, nxt = (int(x) for x in e[1:].split(":"))
                assert nxt == act[act.index(l) + 1] and all(t >= c["nslot"] for t in c["chunks"])
                seen += nxt > l + 1
    assert seen, "a run-ahead across a skipped layer"


def run_launch(c, cnt, epoch, order):
    """the workgroups of one row block in `order`, each blocking at its waits; returns False when no workgroup can move"""
    progs = {}
    for w in c["wgs"]:
        waits = {int(e[1:].split(":")[0]): int(e.split(":")[1]) for e in w["L"] if e[0] == "W"}
        prog = []
        for l in layers_of(w["M"]):
            if l in waits:
                assert waits[l] == l - 1, "a wait is on the layer before"
                prog.append(("W", l - 1))
            if "A%d" % l in w["M"]:
                prog.append(("A", l))
        assert (w["first"] > 0) == (bool(prog) and prog[0] == ("W", w["first"] - 1)), "a first active layer > 0 polls like any consumer"
        progs[w["tn"]] = prog
    pc = {tn: 0 for tn in progs}
    while any(pc[tn] < len(progs[tn]) for tn in progs):
        moved = False
        for tn in order:
            while pc[tn] < len(progs[tn]):
                kind, l = progs[tn][pc[tn]]
                if kind == "W" and ((cnt[l] - c["targets"][(l, epoch)]) & 0xffffffff) >= 0x80000000:
                    break  # (the kernel's comparison: (int)(v - target) >= 0)
                if kind == "A":
                    cnt[l] = (cnt[l] + 1) & 0xffffffff
                pc[tn] += 1
                moved = True
        if not moved:
            return False
    return True


def test_every_counter_receives_its_layer_s_column_tiles_and_the_launch_makes_progress(cases):
    for c in cases:
        grid = max(c["tiles"])
        for order in (list(range(grid)), list(range(grid))[::-1]):
            cnt = [0] * c["L"]
            for epoch in (1, 2, 3):  # several launches of one chain on one key
                assert run_launch(c, cnt, epoch, order), (c["tiles"], order)
                assert cnt == [epoch * c["tiles"][l] if l + 1 < c["L"] else 0 for l in range(c["L"])], (c["tiles"], epoch, cnt)


def test_targets_in_wrap_around_arithmetic(cases):
    for c in cases:
        for (l, e), v in c["targets"].items():
            assert v == (e * c["tiles"][l]) & 0xffffffff


def test_two_chains_alternate_on_one_key_and_chains_of_other_inner_widths_need_their_own(cases):
    by = {(c["tile"], tuple(c["tiles"])): c for c in cases}
    for t in range(4):
        a = by[(t, (3, 1, 3))]
        cnt = [0, 0, 0]
        for epoch in (1, 2):  # (two chains of the SAME widths share a block: the epochs count their launches together)
            assert run_launch(a, cnt, epoch, [0, 1, 2])
        b = by[(t, (1, 3, 3))]  # one grid, one layer count, other inner widths: as launch 3 on a's counters both of its targets would be wrong
        assert max(a["tiles"]) == max(b["tiles"]) and a["L"] == b["L"]
        assert all(b["targets"][(l, 3)] != cnt[l] + b["tiles"][l] for l in range(2))
        assert run_launch(a, cnt, 3, [2, 1, 0]) and cnt == [9, 3, 0]
        own = [0, 0, 0]
        for epoch in (1, 2, 3):
            assert run_launch(b, own, epoch, [2, 1, 0])
