"""CPU check of the maps of a layer chain on the 256x256 bf16 tile (tpp-mlir_amd/csrc/brgemm_bf16_dma256_chain.h with the step walk of
brgemm_bf16_lw_chain_rounds.h; xsmm_hip_set_chain_dma256): the header the kernel, its launcher and the planner include, compiled as plain host
C++ with tests/chain_dma256_schedule/driver.cpp. For a spread of (tiles_m, tiles_n, G, L): the workgroup map - the linear one and the
XCD-blocked one - is a bijection onto G x tiles_n, every tile of every layer is computed exactly once, every counter cnt[l][tm] receives
exactly tiles_n arrivals per launch, and a simulated execution in which every workgroup is resident and a step runs only when its counter
has reached its target completes - in the identity order of the workgroups and in the reversed one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
# (tiles_m, tiles_n, G, L): one workgroup; the GPU test's grids (one round linear and XCD-blocked, forced G even, uneven and 1); the rows of the
# A/B - 64 x 4 in one round, 128 x 4 in two, 16 x 16 -; odd counts; G not dividing tiles_m; eight layers
CASES = [(1, 1, 1, 3), (2, 2, 2, 3), (3, 2, 3, 3), (4, 2, 4, 3), (5, 1, 2, 3), (4, 2, 2, 3), (3, 1, 1, 3), (264, 1, 132, 2), (64, 4, 64, 3), (128, 4, 64, 3),
         (16, 16, 16, 3), (32, 4, 32, 3), (7, 3, 3, 2), (9, 5, 4, 8), (12, 6, 8, 4), (12, 6, 5, 4), (64, 4, 1, 2), (20, 2, 12, 5)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("chain_dma256_schedule") / "walk")
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O2", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "chain_dma256_schedule", "driver.cpp"), "-o", out])
    return out


def facts(exe, *args):
    out = {}
    for l in subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = l.split()
        out[f[0]] = f[1:]
    return out


@pytest.mark.parametrize("order", [0, 1], ids=["identity", "reversed"])
@pytest.mark.parametrize("tiles_m,tiles_n,G,L", CASES)
def test_the_walk_computes_every_tile_once_and_completes(exe, tiles_m, tiles_n, G, L, order):
    f = facts(exe, tiles_m, tiles_n, G, L, order)
    blocked = int(G % 4 == 0 and tiles_n % 2 == 0)
    assert f["map"] == [str(G * tiles_n), "bijection", "1", "groups_seen", str(G), "cols_seen", str(tiles_n), "blocked", str(blocked)], f["map"]
    assert f["tiles"] == ["once", str(L * tiles_m * tiles_n), "never", "0", "more", "0"], f["tiles"]
    assert f["arrivals"] == ["exact", str((L - 1) * tiles_m), "other", "0"], f["arrivals"]
    assert f["run"][:4] == ["done", "1", "steps", str(L * tiles_m * tiles_n)], f["run"]


def test_both_forms_of_the_map_are_among_the_cases():
    assert {int(G % 4 == 0 and tn % 2 == 0) for _, tn, G, _ in CASES} == {0, 1}
    assert any(tm % G for tm, _, G, _ in CASES), "groups owning unequal numbers of row blocks"


def test_what_the_launcher_refuses_is_refused(exe):
    for args in ((4, 2, 5, 3, 0), (4, 2, 0, 3, 0), (4, 2, 2, 1, 0), (4, 2, 2, 9, 0), (0, 2, 1, 3, 0)):
        assert subprocess.run([exe] + [str(a) for a in args], capture_output=True).returncode == 3, args
