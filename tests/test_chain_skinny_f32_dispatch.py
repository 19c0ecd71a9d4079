"""The skinny-batch f32 chain form of the layer-chain launch decision (rt_chain.h try_chain_launch, case CF_SKINNY_F32;
xsmm_hip_set_chain_skinny_f32) on a CPU: tests/chain_skinny_f32_dispatch/driver.cpp links runtime.cpp, host_cache.cpp, gemm_plan.cpp,
tests/chain_dispatch/fake_chain.cpp and tests/chain_skinny_dispatch/fake_skinny_chain.cpp - all compiled unchanged - with
fake_skinny_f32_chain.cpp, which defines launch_f32_skinny_chain as an oracle stand-in with a model of the seam counters (in the other host
builds of runtime.cpp its weak refusing stand-in is linked). tests/test_chain_skinny_f32_cpu.py walks the schedule and asks plan_chain and
stops there; tests/test_chain_skinny_f32_gpu.py starves nothing. What lies between the plan and the kernel is here.
  args       the six chains of tests/test_chain_skinny_f32_cpu.py chains(bn) at BN 16 / 32 / 64 and m 1 / 16 / 17 / 31 under a forced BN, the
             forced_G chain under G 1 / 3 / 7, a chain of 65 column blocks of BN 16 (G capped at 64 compute units): the argument block is the
             calls' - pointers, leading dimensions, strides, k, br, epilogue bits, pad = n_l, groups = G -, target = epoch * G growing by G per
             launch of a counter block, exactly the new counter moves and reads (G, BN, the deepest layer's waves), and the one launch equals
             the calls one by one bit for bit through the oracle
  sequence   an f32 skinny chain, a bf16 skinny chain and a plain bf16 chain of one row block with the same G and layer count share a counter
             block (tests/test_chain_skinny_f32_gpu.py relies on the f32 / bf16 sharing); interleaved in shuffled order over six epochs none
             of the three stand-ins ever sees an unexpected counter
  probation  a starved first launch - the stand-in sets the error word; nothing is provoked on a GPU - degrades to call by call, and so
             does every later chain invoke of the process
  sanitizers the same driver built once more with -fsanitize=address,undefined as a stand-alone program (nothing is loaded into Python)

Shown to fail once, on scratch copies of rt_chain.h (never committed), each built and run as this file builds and runs the driver:
  pad left 0 for CF_SKINNY_F32                        args, sequence and probation red: the stand-in refuses as the launcher does (skf_shape_ok
                                                      of n = 0) and the runtime ends the process at the failed launch
  target = epoch * nlayers instead of epoch * G       args red (TARGET and COUNTER MODEL lines wherever G is not the layer count); sequence,
                                                      two layers on G = 2, stays green - there the two products are the same number
  the third counter word from layer 0 alone           args and sequence red (STATS lines: ragged_k, waves_1_8, the sequence's chain - every
                                                      chain whose first layer is not its deepest)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = "/opt/rocm/include"
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
SOURCES = [os.path.join(CSRC, "runtime.cpp"), os.path.join(CSRC, "host_cache.cpp"), os.path.join(CSRC, "gemm_plan.cpp"),
           os.path.join(ROOT, "tests", "chain_dispatch", "fake_chain.cpp"), os.path.join(ROOT, "tests", "chain_skinny_dispatch", "fake_skinny_chain.cpp"),
           os.path.join(ROOT, "tests", "chain_skinny_f32_dispatch", "fake_skinny_f32_chain.cpp"), os.path.join(ROOT, "tests", "chain_skinny_f32_dispatch", "driver.cpp")]
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
    exe, log = build(str(tmp_path_factory.mktemp("chain_skinny_f32_dispatch")), "driver", [])
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
def test_the_argument_block_the_target_the_counter_and_the_bits(driver, cus):
    passed(*run(driver, ["args"], cus))


def test_an_f32_skinny_a_bf16_skinny_and_a_plain_chain_share_a_counter_block(driver):
    rc, out, err = run(driver, ["sequence"])
    print(out[-1500:])
    passed(rc, out, err)
    assert "sequence: 18 launches, shared block 1, 0 + 0 + 0 counter mismatches" in out


def test_a_starved_first_launch_runs_call_by_call_and_turns_chains_off(driver):
    rc, out, err = run(driver, ["probation"])
    passed(rc, out, err)
    assert "the first fused-brgemm chain launch on this stream was starved" in err and "layer 1's input" in err and "call by call" in err, err[-1500:]


@pytest.mark.timeout(600)
def test_driver_under_asan_and_ubsan(tmp_path):
    """the same sources as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: a reduced args pass with the sequence,
    and the probation. Leak detection off: handles and counter blocks live as long as the process."""
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
