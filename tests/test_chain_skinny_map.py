"""CPU walk of the schedule of the skinny-batch layer chain (tpp-mlir_amd/csrc/brgemm_bf16_skinny_chain.h; xsmm_hip_set_chain_skinny): the header the
kernel, its launcher and the planner include, compiled as plain host C++ with tests/chain_skinny_map/driver.cpp. For G = 1 .. 9, BN = 16 /
32 / 64 and chains of 2 .. 4 layers with 1 .. 20 column blocks, mixed per layer: every (layer, block) has exactly one owner, every seam
receives exactly G arrivals, the deal over a layer's waves is the single call's, every column is stored exactly once - the shifted last
block included - and a simulation of the waits ends under every workgroup order tried, over three launches on the same counters."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++")
    if not cc:
        pytest.skip("needs a host C++ compiler")
    out = str(tmp_path_factory.mktemp("chain_skinny_map") / "walk")
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O2", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "chain_skinny_map", "driver.cpp"), "-o", out])
    return out


def test_the_schedule_walks_clean(walk):
    r = subprocess.run([walk], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    counts = [int(x.split()[-1]) for x in r.stdout.splitlines()[-2].split(",")]
    assert all(c > 0 for c in counts), counts
