"""CPU check of the schedule of a ragged mixed-width layer chain (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_wragged.h,
xsmm_hip_set_chain_widths_ragged, launch mode 11 of the bf16 loader-wave tile): the header the chain kernel's loader and MFMA waves, its
launcher and the planner include, compiled as plain host C++ with tests/chain_wragged_schedule/driver.cpp. For every tile 0 .. 3 and a
list of shapes - sit out and resume, a first active layer > 0, a last active layer that is not the chain's last, n = 2 BN next to 2 BN + 8,
m in {BM + 8, 3 BM - 3, 2 BM}, every skip count 1 .. 7, a 12-chunk layer, eight layers - the driver walks every workgroup's loader role and
MFMA role and checks: every element of every layer is stored by exactly one workgroup and nothing outside a window; every k-value of every
batch element is multiplied exactly once; both roles agree on every chunk's ring slot and no slot is refilled before its chunk was
consumed; every counter receives exactly ceil(n(l) / BN) arrivals per row block and launch; the targets hold over three epochs across an
unsigned wrap; and a round-robin run of all workgroups with the waits as specified completes, in two orders (the acyclicity proof)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

BM = [32, 64, 64, 128]
BN = [64, 64, 128, 128]
SHAPES = ["sitout-resume", "sitout-resume-3bm-3", "first-active-later", "first-active-later-3bm-3", "2bn-next-to-2bn+8", "2bn+8-next-to-2bn", "k72", "k80", "k88",
          "k96", "k104", "k112", "k120", "k200", "ragged-m-only", "twelve-chunks", "eight-layers", "two-batch-elements"]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("chain_wragged_schedule") / "schedule")
    subprocess.check_call([cc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "chain_wragged_schedule", "driver.cpp"), "-o", exe])
    r = dict(cases=[], fails=[], arrivals=[], seen={}, ok={}, inst=None, table=None)
    for line in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = line.split()
        if f[0] == "case":
            L = int(f[4])
            r["cases"].append(dict(tile=int(f[1]), name=f[2], m=int(f[3]), L=L, n=[int(x) for x in f[5:5 + L]], k=[int(x) for x in f[5 + L:5 + 2 * L]],
                                   br=[int(x) for x in f[5 + 2 * L:5 + 3 * L]]))
        elif f[0] == "fail":
            r["fails"].append(line)
        elif f[0] == "arrivals":
            r["arrivals"].append((int(f[1]), f[2], int(f[3]), int(f[4]), int(f[5]), int(f[6])))
        elif f[0] == "seen":
            r["seen"][f[1]] = int(f[2])
        elif f[0] == "ok":
            r["ok"][f[1]] = int(f[2])
        elif f[0] == "inst":
            r["inst"] = [tuple(int(x) for x in i.split(":")) for i in f[1:]]
        elif f[0] == "table":
            r["table"] = [int(x) for x in f[1:]]
    return r


def test_the_case_list_is_the_issue_s(out):
    assert len(out["cases"]) == 4 * len(SHAPES)
    for t in range(4):
        mine = [c for c in out["cases"] if c["tile"] == t]
        assert [c["name"] for c in mine] == SHAPES
        by = {c["name"]: c for c in mine}
        assert by["sitout-resume"]["n"] == [3 * BN[t] + 8, BN[t] + 8, 2 * BN[t] + 24] and by["sitout-resume"]["m"] == BM[t] + 8
        assert by["first-active-later"]["n"] == [BN[t] + 8, 3 * BN[t], BN[t] + 16]
        assert by["2bn-next-to-2bn+8"]["n"][:2] == [2 * BN[t], 2 * BN[t] + 8] and by["2bn+8-next-to-2bn"]["n"][:2] == [2 * BN[t] + 8, 2 * BN[t]]
        assert {c["m"] for c in mine} == {BM[t] + 8, 3 * BM[t] - 3, 2 * BM[t]}
        assert [by["k%d" % k]["k"][0] for k in (72, 80, 88, 96, 104, 112, 120, 200)] == [72, 80, 88, 96, 104, 112, 120, 200]
        assert by["twelve-chunks"]["k"][0] == 200 and by["twelve-chunks"]["br"][0] == 3
        assert by["eight-layers"]["L"] == 8
        assert by["two-batch-elements"]["br"] == [2, 2, 2]
        for c in mine:
            assert len(set(c["n"])) > 1, "at least two widths"


def test_no_property_of_the_schedule_fails(out):
    """stores exactly once and inside the windows, k-values exactly once, ring slots agreed and never refilled early, arrivals, targets,
    and the round-robin run completes"""
    assert out["fails"] == []


def test_every_counter_receives_ceil_n_over_bn_arrivals(out):
    assert out["arrivals"]
    by = {(c["tile"], c["name"]): c for c in out["cases"]}
    for tile, name, l, tm, got, want in out["arrivals"]:
        c = by[(tile, name)]
        assert want == (-(-c["n"][l] // BN[tile]) if l + 1 < c["L"] else 0) and got == want, (tile, name, l, tm)
        assert 0 <= tm < -(-c["m"] // BM[tile])


def test_the_shape_list_exercises_every_mechanism(out):
    seen = out["seen"]
    for what in ["sit-out-and-resume", "first-active-layer-later", "last-active-layer-not-the-chain-s-last", "shifted-in-one-layer-interior-in-another",
                 "shifted-column-tile", "ragged-m", "two-counter-wait", "twelve-chunk-layer", "eight-layers", "epoch-wraps", "layer-starts-at-a-later-slot",
                 "layer-starts-at-an-odd-slot"] + ["skip-%d" % s for s in range(1, 8)]:
        assert seen.get(what, 0) > 0, what


def test_the_launcher_s_refusals_one_accepted_launch_and_one_refusal_per_term(out):
    ok = out["ok"]
    accepted = ["accepted", "its-flat-instance", "ragged-m-alone", "ragged-k-alone", "ragged-n-alone"]
    refused = ["tile-4", "b-kind-1", "no-instance", "one-layer", "nine-layers", "empty-batch", "k-below-64", "k-not-a-multiple-of-8", "n-below-bn", "n-not-a-multiple-of-8",
               "equal-widths", "m-below-bm", "divided-entirely"]
    assert {t: ok[t] for t in accepted} == {t: 1 for t in accepted}
    assert {t: ok[t] for t in refused} == {t: 0 for t in refused}
    assert sorted(out["inst"]) == sorted((t, b) for t in range(4) for b in (0, 2, 4) if (t, b) != (2, 0)) and len(out["inst"]) == 11
    assert out["table"] == [8, 11, 0, 0], "BLW_MODES stays 8; the launch table goes on refusing mode 11"
