"""The epilogue fold's eligibility rules on the host (no GPU): runtime.cpp compiled unchanged against tests/tsan/fake_hip.cpp plus the
host stand-in of the epilogue launcher (tests/fold_host/driver.cpp), driven by hand-built invoke sequences. Each case must give the same
bytes with the fold on and off, and the expected folded / declined / ended-group decisions."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = "/opt/rocm/include"


@pytest.mark.timeout(600)
def test_fold_decisions_on_hand_built_sequences(tmp_path):
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "fold_driver")
    cmd = [gxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE,
           os.path.join(ROOT, "tpp-mlir_amd", "csrc", "runtime.cpp"), os.path.join(ROOT, "tpp-mlir_amd", "csrc", "host_cache.cpp"),
           os.path.join(ROOT, "tests", "tsan", "fake_hip.cpp"), os.path.join(ROOT, "tests", "fold_host", "driver.cpp"),
           "-o", exe, "-pthread", "-ldl"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ)
    for k in ("TPP_HIP_ASYNC", "TPP_HIP_TILE_QUEUE", "TPP_HIP_TRACE", "TPP_HIP_VARIANT", "TPP_HIP_FOLD_EPILOGUE", "TPP_HIP_STRICT"):
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and out.strip().endswith("OK"), out[-4000:]
