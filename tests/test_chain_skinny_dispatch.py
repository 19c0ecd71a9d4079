"""The skinny-batch chain form of the layer-chain launch decision (rt_chain.h try_chain_launch, case CF_SKINNY; xsmm_hip_set_chain_skinny) on a
CPU: tests/chain_skinny_dispatch/driver.cpp links runtime.cpp, host_cache.cpp, gemm_plan.cpp and tests/chain_dispatch/fake_chain.cpp - all
compiled unchanged - with fake_skinny_chain.cpp, which defines launch_bf16_skinny_chain as an oracle stand-in with a model of the seam counters
(in the other host builds of runtime.cpp its weak refusing stand-in is linked).
  args       the argument block is the calls' - pointers, leading dimensions, strides, k, br, epilogue bits, pad = n_l, groups = G -, exactly
             the new counter moves and describes the launch, and the one launch equals the calls one by one bit for bit through the oracle
  sequence   a skinny chain and a plain chain of one row block with the same G and layer count share a counter block (the choice stated in
             brgemm_bf16_skinny_chain.h); interleaved in shuffled order over six epochs neither ever sees an unexpected counter
  probation  a starved first launch - the stand-in sets the error word; nothing is provoked on a GPU - degrades to call by call
  sanitizers the same driver built once more with -fsanitize=address,undefined as a stand-alone program (nothing is loaded into Python)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = "/opt/rocm/include"
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
SOURCES = [os.path.join(CSRC, "runtime.cpp"), os.path.join(CSRC, "host_cache.cpp"), os.path.join(CSRC, "gemm_plan.cpp"),
           os.path.join(ROOT, "tests", "chain_dispatch", "fake_chain.cpp"), os.path.join(ROOT, "tests", "chain_skinny_dispatch", "fake_skinny_chain.cpp"),
           os.path.join(ROOT, "tests", "chain_skinny_dispatch", "driver.cpp")]
ORACLE = os.path.join(ROOT, "oracle", "xsmm_oracle.c")
RUN_TIMEOUT = 240


def build(out_dir, name, flags):
    """every translation unit compiled on its own, side by side, then one link; returns (exe, None) or (None, compiler output)"""
    gxx, gcc = shutil.which("g++"), shutil.which("gcc")
    if not gxx or not gcc or not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime.h")):
        pytest.skip("needs g++, gcc and the HIP headers")
    jobs, objs = [], []
    for src in SOURCES + [ORACLE]:
        obj = os.path.join(out_dir, name + "_" + os.path.basename(src) + ".o")
        objs.append(obj)
        cc = [gcc, "-O2"] if src.endswith(".c") else [gxx, "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE]
        jobs.append(subprocess.Popen(cc + flags + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [j.communicate()[0] for j in jobs]
    if any(j.returncode for j in jobs):
        return None, "\n".join(logs)
    exe = os.path.join(out_dir, name)
    link = subprocess.run([gxx] + flags + objs + ["-o", exe, "-pthread", "-ldl", "-lm"], capture_output=True, text=True)
    return (exe, None) if link.returncode == 0 else (None, link.stdout + link.stderr)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe, log = build(str(tmp_path_factory.mktemp("chain_skinny_dispatch")), "driver", [])
    assert exe, log[-4000:]
    return exe


def run(exe, args, cus=256, extra_env=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_") and k != "LD_PRELOAD"}
    env.update(extra_env or {}, FAKE_HIP_CUS=str(cus))
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=RUN_TIMEOUT)
    return r.returncode, r.stdout, r.stderr


def passed(rc, out, err):
    assert rc == 0 and out.strip().endswith("OK") and "FAIL" not in out and "COUNTER MODEL" not in err, (out[-6000:], err[-3000:])


@pytest.mark.parametrize("cus", [256, 64])
def test_the_argument_block_the_counter_and_the_bits(driver, cus):
    passed(*run(driver, ["args"], cus))


def test_a_skinny_chain_and_a_plain_chain_share_a_counter_block(driver):
    rc, out, err = run(driver, ["sequence"])
    print(out[-1500:])
    passed(rc, out, err)
    assert "shared block 1, 0 + 0 counter mismatches" in out


def test_a_starved_first_launch_runs_call_by_call_and_turns_chains_off(driver):
    rc, out, err = run(driver, ["probation"])
    passed(rc, out, err)
    assert "starved" in err and "call by call" in err, err[-1500:]


@pytest.mark.timeout(600)
def test_driver_under_asan_and_ubsan(tmp_path):
    """the same sources as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer. Leak detection off: handles and
    counter blocks live as long as the process."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    exe, log = build(str(tmp_path), "driver_asan", flags)
    if not exe and ("asan" in log.lower() or "ubsan" in log.lower()):
        pytest.skip("this compiler has no ASan / UBSan runtime")
    assert exe, log[-4000:]
    env = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    for args in (["sanitize"], ["probation"]):
        rc, out, err = run(exe, args, extra_env=env)
        assert "AddressSanitizer" not in out + err and "runtime error:" not in out + err, (out + err)[-6000:]
        passed(rc, out, err)
