"""CPU checks of launch mode 10 of the bf16 loader-wave tile (BLW_CHAIN_WROUNDS, tpp-mlir_amd/csrc/brgemm_bf16_lw_launch.h): what
blw_chain_wrounds_launch_ok takes and refuses - one accepted launch and one refusal per term -, which instances
blw_chain_wrounds_instance_exists names, that the mode stays beside the launch table (BLW_MODES is 8, blw_instance_exists and blw_launch_ok
refuse it) - and, compile-only, that brgemm_bf16_lw_chain_wrounds.hip holds exactly those instances, none with scratch."""
import subprocess

import pytest

import chain_width_rounds_codeobj as codeobj
from test_chain_width_rounds_schedule import compile_driver


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = compile_driver(tmp_path_factory.mktemp("chain_width_rounds_launch"))
    out = {"ok": {}}
    for line in subprocess.run([exe, "launch"], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines():
        f = line.split()
        if f[0] == "ok":
            out["ok"][f[1]] = int(f[2])
        elif f[0] == "inst":
            out["inst"] = [tuple(int(x) for x in i.split(":")) for i in f[1:]]
        elif f[0] == "table":
            out["table"] = [int(x) for x in f[1:]]
    return out


def test_the_launcher_takes_one_launch_and_refuses_one_per_term(answers):
    terms = ["tile-4", "b-kind-1", "one-layer", "nine-layers", "empty-batch", "k-below-64", "k-not-in-chunks", "n-below-bn", "n-not-in-tiles", "equal-widths", "m-below-bm",
             "m-not-in-blocks", "groups-zero", "groups-negative", "groups-widest", "groups-above-widest"]
    ok = answers["ok"]
    assert ok["accepted"] == 1 and ok["accepted-one-group"] == 1
    assert {t: ok[t] for t in terms} == {t: 0 for t in terms}
    assert len(ok) == len(terms) + 2


def test_the_instances_and_the_mode_s_place_beside_the_table(answers):
    assert sorted(answers["inst"]) == sorted((t, b) for t in range(4) for b in (0, 2, 4)) and len(answers["inst"]) == 12
    assert answers["table"] == [8, 10, 0, 0], "BLW_MODES stays 8; the launch table goes on refusing mode 10"


def test_the_translation_unit_holds_exactly_the_instances_of_its_table_and_no_scratch(answers):
    rep = codeobj.report()
    want = [codeobj.symbol(t, b) for t, b in answers["inst"]]
    assert len(want) <= 12 and sorted(rep) == sorted(want), (sorted(set(rep) - set(want)), sorted(set(want) - set(rep)))
    assert not {n: x for n, x in rep.items() if x[0] or x[1] > 256 or x[2]}, rep
