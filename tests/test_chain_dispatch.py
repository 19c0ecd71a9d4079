"""The layer-chain launch decision (tpp-mlir_amd/csrc/rt_chain.h try_chain_launch) on a CPU, under every combination of the seven chain
switches (no GPU needed). runtime.cpp, host_cache.cpp and the real planner gemm_plan.cpp are compiled UNCHANGED with g++ and linked
against tests/chain_dispatch/fake_chain.cpp - the HIP host entry points over host memory (tests/tsan/fake_hip_host.h, FAKE_HIP_CUS compute
units), launch stand-ins that compute every layer in bf16 through oracle/xsmm_oracle.c from the kernel argument block alone, one record per
launch, and a model of the hand-off counters fed from the project's CPU-walkable schedule headers - and driven through the C-ABI by
tests/chain_dispatch/driver.cpp. One process per (compute units, strict) pair: descriptors are planned once, at dispatch.

  a  switch independence: for every chain of the lattice, every B image and all 128 switch sets S, D(S) is D({}) or the D({x}) of the
     switch of S that wins by ONE precedence list (the 256x256 tile first, a forced 1000 + G / 1000 + W in front of the one-round rules,
     mixed widths in front of column rounds, the one-round ragged launch in front of several rounds, ragged width and then ragged mixed
     widths where the others refuse) - also with the forcing values, the forcing edge-tile modes and xsmm_hip_set_dma256_images in the
     set, and the three single-call ragged switches change no chain decision. 64 / 256 / 304 compute units, strict off / on.
  b  per launch: grid <= compute units, the tile divides / ceil-divides as the form says, every k meets the form's condition, one B
     image, m / n / nlayers / pad / groups, every pointer, leading dimension, stride, k, batch count and epilogue bit is the call's,
     exactly the form's *_stats counter moved by one and describes the grid. What the rules exclude stays call by call under every set.
  c  marshalling: one small chain per form and image, gap columns behind every row - the one launch equals the calls one by one bit
     for bit (both through the oracle), the NaN pattern in the gap columns survives.
  d  counters: chains whose counter-block keys coincide (plain / edge rows / rounds / ragged width on one grid; mixed widths / column
     rounds / ragged mixed widths on one grid; two mixed-width chains that differ in an inner width only) interleaved in shuffled order
     over several epochs: the counter model never sees a counter that is not expected_after - arrivals.
  e  degrading: per form, a starved FIRST launch (probation) runs call by call and turns chains off; a starved JOURNALED launch and its
     successor are re-run in order at the synchronisation, and xsmm_hip_chain_status counts them. A process each: the flag is sticky.
  f  tests/golden/chain_dispatch.txt: D({}), the seven D({x}) and D(all) per chain, image, compute units and strict mode. A rule change
     shows as a diff of that file. Regenerate: build as below, then `driver table off images` (FAKE_HIP_CUS=256), `driver table off`
     (64, 304) and `driver table strict` (256), concatenated in the order of TABLE_RUNS.
  g  the same driver built once more with -fsanitize=address,undefined as a stand-alone program (nothing is loaded into Python).
The regression case of a: 32 * 257 rows x [64, 64] with a flat or VNNI-4 B and the edge-row and multi-round switches both on ran in two
rounds on the planned 32x64 tile instead of the one-round ragged launch that xsmm_hip_set_chain_edge alone takes ('8224x[64]*3').
Run phase here: a sweep process about 1 s (203 000 invokes), the sequence 7 s, everything else below 4 s; the compile dominates."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = "/opt/rocm/include"
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
SOURCES = [os.path.join(CSRC, "runtime.cpp"), os.path.join(CSRC, "host_cache.cpp"), os.path.join(CSRC, "gemm_plan.cpp"),
           os.path.join(ROOT, "tests", "chain_dispatch", "fake_chain.cpp"), os.path.join(ROOT, "tests", "chain_dispatch", "driver.cpp")]
ORACLE = os.path.join(ROOT, "oracle", "xsmm_oracle.c")
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_dispatch.txt")
FORMS = ["plain", "f32", "edge", "rounds", "ragged", "widths", "wrounds", "wragged", "dma256"]
# (compute units, driver arguments) of the golden table, in file order
TABLE_RUNS = [(256, ["off", "images"]), (64, ["off"]), (304, ["off"]), (256, ["strict"])]
RUN_TIMEOUT = 240  # seconds per driver process; the slowest (the sequence, or a sweep under load) takes well under 10 here


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
    exe, log = build(str(tmp_path_factory.mktemp("chain_dispatch")), "driver", [])
    assert exe, log[-4000:]
    return exe


def run(exe, args, cus=256, extra_env=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_") and k != "LD_PRELOAD"}
    env.update(extra_env or {}, FAKE_HIP_CUS=str(cus))
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=RUN_TIMEOUT)
    return r.returncode, r.stdout, r.stderr


def passed(rc, out, err):
    assert rc == 0 and out.strip().endswith("OK") and "FAIL" not in out and "COUNTER MODEL" not in err, (out[-6000:], err[-3000:])


@pytest.mark.timeout(600)
def test_decision_table_matches_the_golden_file(driver):
    got = ""
    for cus, args in TABLE_RUNS:
        rc, out, err = run(driver, ["table"] + args, cus)
        passed(rc, out, err)
        got += "\n".join(line for line in out.splitlines() if line != "OK") + "\n"
    want = open(GOLDEN).read()
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        diff = [f"- {b}\n+ {a}" for a, b in zip(g, w) if a != b]
        assert False, f"{len(diff)} rows differ (golden -, now +), {len(g)} rows now, {len(w)} in the file:\n" + "\n".join(diff[:12])
    assert 100 < len(want.splitlines()) < 500


@pytest.mark.timeout(600)
@pytest.mark.parametrize("strict", ["off", "strict"])
@pytest.mark.parametrize("cus", [64, 256, 304])
def test_switch_independence_and_launch_invariants(driver, cus, strict):
    rc, out, err = run(driver, ["sweep", strict], cus)
    print(out[-1500:])
    passed(rc, out, err)
    assert f"{cus} compute units, strict {int(strict == 'strict')}" in out
    if cus == 256 and strict == "off":
        # every one of the nine forms launched, with every B image it has (the driver asserts it too: COVERAGE)
        line = [l for l in out.splitlines() if l.startswith("forms launched")][0].split(":", 1)[1].split()
        seen = dict(zip(line[0::2], line[1::2]))
        assert sorted(seen) == sorted(FORMS), seen
        for form, counts in seen.items():
            n = [int(c) for c in counts.split("/")]
            assert n[1] > 0 if form == "f32" else all(c > 0 for c in n), (form, counts)


@pytest.mark.timeout(600)
def test_one_launch_is_the_calls_one_by_one_bit_for_bit(driver):
    rc, out, err = run(driver, ["arith"])
    print(out)
    passed(rc, out, err)
    for form in FORMS:
        assert f"one {form} launch = the calls one by one" in out, form


@pytest.mark.timeout(600)
def test_counter_blocks_shared_between_forms_across_a_shuffled_sequence(driver):
    rc, out, err = run(driver, ["sequence"])
    print(out)
    passed(rc, out, err)
    assert "0 counter mismatches" in out and out.count("share a counter block") >= 10


@pytest.mark.timeout(600)
@pytest.mark.parametrize("form", range(len(FORMS)), ids=FORMS)
def test_a_starved_first_launch_runs_call_by_call_and_turns_chains_off(driver, form):
    rc, out, err = run(driver, ["probation", str(form)])
    passed(rc, out, err)
    assert "starved first launch ran call by call" in out and "the first fused-brgemm chain launch on this stream was starved" in err


@pytest.mark.timeout(600)
def test_a_starved_journaled_launch_and_its_successor_are_rerun_in_order(driver):
    rc, out, err = run(driver, ["journal"])
    passed(rc, out, err)
    assert "status 2" in out and "are re-run call by call now" in err
    # TPP_HIP_CHAIN_STRICT=1 keeps fail-stop: the same scenario ends the process at the synchronisation
    rc, out, err = run(driver, ["journal"], extra_env={"TPP_HIP_CHAIN_STRICT": "1"})
    assert rc != 0 and "TPP_HIP_CHAIN_STRICT=1 asks for fail-stop" in err and "status" not in out, (rc, out, err[-2000:])


@pytest.mark.timeout(600)
def test_a_chain_invoke_asks_for_the_compute_units_at_most_once(driver):
    """h  the stream's compute units cost three runtime calls per question (hipExtStreamGetCUMask is counted): for every chain of the
    lattice under D({}), each D({x}) and D(all), at most one question per invoke, none where the chain contract refuses, none where
    column rounds by rule meet calls that share no tile they were all dispatched on (the mixed-width switch off)."""
    rc, out, err = run(driver, ["cus"])
    print(out[-1500:])
    passed(rc, out, err)
    line = [l for l in out.splitlines() if l.startswith("cus:")][0].split()
    invokes, asked, contract, gated = int(line[1]), int(line[4]), int(line[6]), int(line[13])
    assert 0 < asked <= invokes and contract > 0 and gated > 0, line


@pytest.mark.timeout(600)
def test_driver_under_asan_and_ubsan(tmp_path):
    """the same unchanged sources as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, as test_tsan_scheduler.py
    builds its own: the 1- / 2- / 8- / 9-call chains and one computing chain per form. Leak detection off: handles and counter blocks
    live as long as the process."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    exe, log = build(str(tmp_path), "driver_asan", flags)
    if not exe and ("asan" in log.lower() or "ubsan" in log.lower()):
        pytest.skip("this compiler has no ASan / UBSan runtime")
    assert exe, log[-4000:]
    env = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    for args in (["sanitize"], ["journal"], ["probation", "7"]):
        rc, out, err = run(exe, args, extra_env=env)
        assert "AddressSanitizer" not in out + err and "runtime error:" not in out + err, (out + err)[-6000:]
        passed(rc, out, err)
