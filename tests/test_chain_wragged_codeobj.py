"""Compile-only check of launch mode 11 of the bf16 loader-wave tile (BLW_CHAIN_WRAGGED): brgemm_bf16_lw_chain_wragged.hip holds exactly the
instances blw_chain_wragged_instance_exists names - tiles 0 .. 3 with the three B images, less the 64x128 tile with the VNNI-2 image -, none
with scratch, none above 256 VGPRs, none with AGPRs. The instance list is the schedule driver's (tests/chain_wragged_schedule/driver.cpp
prints the predicate's answers), so the test and the launcher read one table."""
import chain_wragged_codeobj as codeobj
from test_chain_wragged_schedule import out  # noqa: F401  (the module fixture that compiles and runs the driver)


def test_the_translation_unit_holds_exactly_the_instances_of_its_table_and_no_scratch(out):  # noqa: F811
    inst = out["inst"]
    assert (2, 0) not in inst and len(inst) == 11
    rep = codeobj.report()
    want = [codeobj.symbol(t, b) for t, b in inst]
    assert sorted(rep) == sorted(want), (sorted(set(rep) - set(want)), sorted(set(want) - set(rep)))
    assert not {n: x for n, x in rep.items() if x[0] or x[1] > 256 or x[2]}, rep
