"""CPU walk of split_scratch_for (tpp-mlir_amd/csrc/split_scratch.h): the per (device, stream) scratch block every split launch takes - the f32
loader-wave split and tail split, the split of brgemm_bf16_small.hip, the skinny K split. The header is compiled as plain host C++ with
tests/split_scratch/driver.cpp against the fake HIP host entry points (tests/tsan/fake_hip_host.h; no GPU needed). One process, one walk: the
same-stream reuse, the doubling from 1 MiB, the cap at SPLIT_SCRATCH_FLOATS, the refusal beyond SPLIT_MAX_TILES, a stream that is being
captured (nullptr, nothing allocated - the fake's hipStreamIsCapturing answers "none" unless the driver says otherwise), and the 17th
(device, stream) pair. Once more as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: the freed areas of the growth
steps are never touched again. On a GPU the same edges: tests/test_graph_capture_gpu.py (growth under launches in flight, the 17th stream)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = "/opt/rocm/include"
DRIVER = os.path.join(ROOT, "tests", "split_scratch", "driver.cpp")


def build(out, flags):
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE] + flags + [DRIVER, "-o", out, "-pthread"],
                       capture_output=True, text=True)
    return r.returncode == 0, r.stdout + r.stderr


def run(exe, extra_env=None, sanitized=False):
    # (host code over the fake HIP: the program never opens a GPU. The sanitized build runs without LD_PRELOAD, like the other stand-alone
    # sanitizer programs of this suite: a preloaded library in front of the AddressSanitizer runtime makes such a program refuse to start)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_") and not (sanitized and k == "LD_PRELOAD")}
    env.update(extra_env or {})
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-3000:]
    return r.stdout, r.stderr


def test_the_walk_of_the_scratch_blocks(tmp_path):
    ok, log = build(str(tmp_path / "walk"), [])
    assert ok, log[-4000:]
    out, _ = run(str(tmp_path / "walk"))
    for step in ("first use:", "growth:", "cap:", "tiles:", "capture:", "pairs:"):
        assert step in out, step
    checks, failed = (int(x) for x in out.splitlines()[-2].replace(" checks,", "").replace(" failed", "").split())
    assert checks > 0 and failed == 0  # (a step's line is printed behind its checks: all six lines = no step was skipped)


def test_the_walk_under_asan_and_ubsan(tmp_path):
    ok, log = build(str(tmp_path / "walk_asan"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if not ok and ("asan" in log.lower() or "ubsan" in log.lower()):
        pytest.skip("this compiler has no ASan / UBSan runtime")
    assert ok, log[-4000:]
    out, err = run(str(tmp_path / "walk_asan"), {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"},
                   sanitized=True)
    assert "AddressSanitizer" not in out + err and "runtime error:" not in out + err, (out + err)[-6000:]
