"""CPU check of the schedule of a mixed-width layer chain in column rounds (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_wrounds.h,
xsmm_hip_set_chain_width_rounds): the header the chain kernel's loader and MFMA waves, its launcher and the planner include, compiled as
plain host C++ with tests/chain_width_rounds_schedule/driver.cpp. For every tile 0 .. 3, the width vectors below (in column tiles, up to
eight layers) and every W from 1 to max T - 1 - among them W that do not divide a T_l ([4, 1, 2] with 3, [5, 2, 7, 3]) and W larger than a
narrow layer's T_l - the driver walks every column group's loader role and MFMA role. Every (layer, tm, tn) is computed exactly once, by
the group the maps name; both roles make the same steps and execute the same barriers; every counter cnt[l][tm] receives exactly T_l
arrivals; a launch in which every workgroup advances only when its wait is satisfied runs to the end from every order tried; the ring
slot of every step follows chain_widths_next_s0; at W = max T the walk is the one-round mixed-width chain's."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

VECTORS = [[4, 1, 2], [1, 3, 1], [2, 1] * 4, [2, 2, 1], [3, 1], [4, 2], [1, 4, 1], [8, 4, 2, 1], [5, 2, 7, 3], [1, 2, 4]]
BARRIERS = ("P", "m", "R1", "S1")


def compile_driver(tmp):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp / "schedule")
    subprocess.check_call([cc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "chain_width_rounds_schedule", "driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    exe = compile_driver(tmp_path_factory.mktemp("chain_width_rounds_schedule"))
    cases, groups, cur = [], [], None
    for line in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = line.split()
        if f[0] == "case":
            tile, nslot, wk, nla, L, W = (int(x) for x in f[1:7])
            cur = dict(tile=tile, nslot=nslot, wk=wk, nla=nla, L=L, W=W, tiles=[int(x) for x in f[7:7 + L]], chunks=[int(x) for x in f[7 + L:7 + 2 * L]], wgs=[])
            cases.append(cur)
        elif f[0] == "wg":
            cur["wgs"].append(dict(c=int(f[1]), steps=[int(x) for x in f[3:]]))
        elif f[0] in ("L", "M"):
            cur["wgs"][-1][f[0]] = f[1:]
        elif f[0] == "groups":
            groups.append(tuple(int(x) for x in f[1:]))
    return cases, groups


@pytest.fixture(scope="module")
def cases(walked):
    return walked[0]


def steps_of(events):
    """[(layer, tn, slot)] of a role"""
    return [tuple(int(x) for x in e[1:].split(":")) for e in events if e[0] == "s"]


def barriers(events):
    return [e for e in events if e.split(":")[0] in BARRIERS]


def test_the_case_list(cases):
    for t in range(4):
        mine = [c for c in cases if c["tile"] == t]
        assert [(c["tiles"], c["W"]) for c in mine] == [(v, w) for v in VECTORS for w in range(1, max(v) + 1)]
    assert {c["wk"] for c in cases} == {1, 2}, "tiles with and without the K-split barrier R1"
    assert max(c["L"] for c in cases) == 8
    assert any(c["W"] < max(c["tiles"]) and any(t % c["W"] for t in c["tiles"] if t > c["W"]) for c in cases), "a W that does not divide a T_l"
    assert any(min(c["tiles"]) < c["W"] < max(c["tiles"]) for c in cases), "a W larger than a narrow layer's T_l"


def test_every_tile_is_computed_exactly_once_by_the_group_the_maps_name(cases):
    for c in cases:
        seen = {}
        for w in c["wgs"]:
            assert steps_of(w["L"]) == steps_of(w["M"]), "both roles make the same steps at the same ring slots"
            per_layer = [0] * c["L"]
            order = [(l, tn) for l, tn, _ in steps_of(w["M"])]
            assert order == sorted(order), "layer-major, column tiles ascending"
            for l, tn, _ in steps_of(w["M"]):
                assert tn % c["W"] == w["c"] and tn == w["c"] + per_layer[l] * c["W"], "chain_wrounds_group / chain_wrounds_tile"
                per_layer[l] += 1
                assert (l, tn) not in seen
                seen[(l, tn)] = w["c"]
            assert per_layer == w["steps"] == [len(range(w["c"], t, c["W"])) for t in c["tiles"]], "chain_wrounds_steps"
        assert sorted(seen) == [(l, tn) for l in range(c["L"]) for tn in range(c["tiles"][l])], (c["tiles"], c["W"])


def test_both_roles_execute_the_same_barriers(cases):
    for c in cases:
        for w in c["wgs"]:
            bm = barriers(w["M"])
            if c["wk"] > 1 and bm and bm[-1] == "R1:%d" % (c["L"] - 1):
                bm = bm[:-1]  # (the chain's very last step: the loaders have ended in front of its R1 - ended waves take no part in barriers)
            assert barriers(w["L"]) == bm, (c["tile"], c["tiles"], c["W"], w["c"])
            # per step: P, one barrier per further chunk, R1 on a K-split tile, S1 unless it is the walk's last step of the last layer
            ev, i = w["M"], 0
            st = steps_of(ev)
            for j, (l, tn, _) in enumerate(st):
                last_of_all = l + 1 == c["L"] and tn + c["W"] >= c["tiles"][l]
                want = ["P:%d" % l] + ["m:%d" % l] * (c["chunks"][l] - 1) + (["R1:%d" % l] if c["wk"] > 1 else []) + ([] if last_of_all else ["S1:%d" % l])
                i = ev.index("s%d:%d:%d" % st[j])
                end = ev.index("s%d:%d:%d" % st[j + 1]) if j + 1 < len(st) else len(ev)
                assert barriers(ev[i:end]) == want


def test_the_ring_slot_of_every_step_follows_chain_widths_next_s0(cases):
    for c in cases:
        for w in c["wgs"]:
            s0 = 0
            for l, tn, slot in steps_of(w["M"]):
                assert slot == s0, (c["tiles"], c["W"], w["c"], l, tn)
                s0 = (s0 + c["chunks"][l]) % c["nslot"]  # (a sat-out layer takes no slot)


def test_a_wait_stands_in_front_of_every_step_of_a_later_layer_and_an_arrival_behind_every_step_but_the_last_layer_s(cases):
    for c in cases:
        for w in c["wgs"]:
            for role, mark in (("L", "W"), ("M", "A")):
                ev = w[role]
                for j, e in enumerate(ev):
                    if e[0] != "s":
                        continue
                    l = int(e[1:].split(":")[0])
                    if role == "L":
                        assert (ev[j + 1] == "W%d" % l) == (l > 0)
                    else:
                        nxt = next((k for k in range(j + 1, len(ev)) if ev[k][0] == "s"), len(ev))
                        assert (("A%d" % l) in ev[j:nxt]) == (l + 1 < c["L"])
                        if l + 1 < c["L"]:
                            assert ev[nxt - 2:nxt] == ["S1:%d" % l, "A%d" % l], "the arrival is the last thing of the step, behind S1"


def test_the_run_ahead_targets_the_next_step(cases):
    same, across, skipped = 0, 0, 0
    for c in cases:
        for w in c["wgs"]:
            st = steps_of(w["L"])
            marks = [e for e in w["L"] if e[0] == "I"]
            if not all(t >= c["nslot"] for t in c["chunks"]):
                assert not marks
                continue
            assert len(marks) == len(st) - 1, "every step but the walk's last runs ahead"
            for j, e in enumerate(marks):
                nl, ntn = (int(x) for x in e[1:].split(":"))
                assert (nl, ntn) == st[j + 1][:2]
                same += nl == st[j][0]
                across += nl == st[j][0] + 1
                skipped += nl > st[j][0] + 1
    assert same and across and skipped, "into the same layer, into the next, across a sat-out layer"


def run_launch(c, cnt, epoch, order, one_event_per_turn=False):
    """the workgroups of one row block, taken in `order` again and again, each blocking at its waits; False when no workgroup can move"""
    progs = {}
    for w in c["wgs"]:
        prog = []
        waits = iter([int(e[1:]) for e in w["L"] if e[0] == "W"])
        for e in w["M"]:
            if e[0] == "s":
                l = int(e[1:].split(":")[0])
                if l > 0:
                    assert next(waits) == l
                    prog.append(("W", l - 1))
            elif e[0] == "A":
                prog.append(("A", int(e[1:])))
        progs[w["c"]] = prog
    pc = {g: 0 for g in progs}
    while any(pc[g] < len(progs[g]) for g in progs):
        moved = False
        for g in order:
            while pc[g] < len(progs[g]):
                kind, l = progs[g][pc[g]]
                if kind == "W" and ((cnt[l] - epoch * c["tiles"][l]) & 0xffffffff) >= 0x80000000:
                    break  # (the kernel's comparison: (int)(v - chain_widths_target) >= 0)
                if kind == "A":
                    cnt[l] = (cnt[l] + 1) & 0xffffffff
                pc[g] += 1
                moved = True
                if one_event_per_turn:
                    break
        if not moved:
            return False
    return True


def test_every_counter_receives_t_l_arrivals_and_the_launch_ends_from_every_order_tried(cases):
    rng = random.Random(20261019)
    for c in cases:
        if c["W"] == max(c["tiles"]):
            continue
        fwd = list(range(c["W"]))
        shuffled = fwd[:]
        rng.shuffle(shuffled)
        for order in (fwd, fwd[::-1], shuffled):
            for single in (False, True):
                cnt = [0] * c["L"]
                for epoch in (1, 2, 3):  # several launches on one counter block
                    assert run_launch(c, cnt, epoch, order, single), (c["tiles"], c["W"], order)
                    assert cnt == [epoch * c["tiles"][l] if l + 1 < c["L"] else 0 for l in range(c["L"])], (c["tiles"], c["W"], epoch, cnt)


def test_at_w_equal_max_t_the_walk_is_the_one_round_chain_s(cases):
    seen = 0
    for c in cases:
        if c["W"] != max(c["tiles"]):
            continue
        seen += 1
        for w in c["wgs"]:
            active = [l for l in range(c["L"]) if w["c"] < c["tiles"][l]]
            assert [(l, tn) for l, tn, _ in steps_of(w["M"])] == [(l, w["c"]) for l in active], "one step per active layer, on column tile c"
            # brgemm_bf16_lw_chain_widths.h: a wait in front of every active layer > 0, the whole seam after every active layer but the last
            assert [int(e[1:]) for e in w["L"] if e[0] == "W"] == [l for l in active if l > 0]
            assert [int(e[1:]) for e in w["M"] if e[0] == "A"] == [l for l in active if l + 1 < c["L"]]
    assert seen == 4 * len(VECTORS)


def test_the_rule_s_w(walked):
    got = {g[:3]: g[3:] for g in walked[1]}
    # (max T, m / BM, compute units) -> (Wfit, W): 1024, 4096 and 2048 rows x [1024, 4096, 1024] on 64x64, 128x128, 128x128
    assert got[(64, 16, 256)] == (16, 16) and got[(32, 32, 256)] == (8, 8) and got[(32, 16, 256)] == (16, 16)
    assert got[(10, 32, 256)] == (8, 5), "two rounds of five, not eight and two"
    assert got[(10, 32, 304)] == (9, 5)
    assert got[(4, 2, 256)] == (3, 2), "a chain that fits in one round: two balanced rounds"
    assert got[(2, 300, 256)] == (0, 0), "more row blocks than compute units"
    assert got[(1, 4, 256)] == (0, 0), "nothing to round"
    assert got[(7, 3, 16)] == (5, 4)
