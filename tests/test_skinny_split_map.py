"""CPU check of the maps of the K split across workgroups of the skinny-batch bf16 kernel (tpp-mlir_amd/csrc/brgemm_bf16_skinny_split.h,
xsmm_hip_set_skinny_split): the header the kernel, its launcher and the planner include, compiled as plain host C++ with
tests/skinny_split_map/driver.cpp.
  - for S_all in 1 .. 70 and 512 steps and P in 2 .. 16: P_eff = min(P, S_all); every step lies in exactly one (part, wave); parts and
    waves are contiguous and in order; the first S_all % P_eff parts take one step more; inside a part the run is dealt exactly as a whole
    call of that many steps is dealt by the unsplit kernel; every part fits the workgroup of part 0 with at most one wave idle, and an idle
    wave has no steps;
  - the linear grid names every (part, column block) exactly once, part-major;
  - every scratch float of a launch is written by exactly one (block, part, register, lane, element) and lies inside the asked size;
    the 64 lanes of one register are 1 KiB contiguous;
  - for br = 3, k = 72 the masked steps of every part are exactly those that end a batch element;
  - the refusal limits are those of split_scratch.h.
The same driver runs once more as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "skinny_split_map", "driver.cpp")
WMAX = 8
STEPS = list(range(1, 71)) + [512]


def compiler():
    return shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"


def limits():
    """(SPLIT_MAX_TILES, SPLIT_MAX, SPLIT_SCRATCH_FLOATS) from the text of split_scratch.h"""
    with open(os.path.join(CSRC, "split_scratch.h")) as f:
        src = f.read()
    tiles = int(re.search(r"constexpr int SPLIT_MAX_TILES = (\d+);", src).group(1))
    parts = int(re.search(r"constexpr int SPLIT_MAX = (\d+);", src).group(1))
    m = re.search(r"constexpr size_t SPLIT_SCRATCH_FLOATS = (\d+)u << (\d+);", src)
    return tiles, parts, int(m.group(1)) << int(m.group(2))


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    """{first word: [fields of every such line as a {name: int} dict]}"""
    exe = str(tmp_path_factory.mktemp("skinny_split_map") / "map")
    subprocess.check_call([compiler(), "-x", "c++", "-std=c++14", "-O2", "-Wall", "-I" + CSRC, DRIVER, "-o", exe])
    out = {}
    for l in subprocess.run([exe] + [str(x) for x in limits()], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = l.split()
        out.setdefault(f[0], []).append({f[i]: int(f[i + 1]) for i in range(1, len(f) - 1, 2)})
    return out


def test_the_limits_restated_here_are_the_headers(facts):
    assert limits() == (4096, 16, 8 << 20)
    assert facts["pmax"] == [dict(value=limits()[1])]
    with open(os.path.join(CSRC, "brgemm_bf16_skinny.h")) as f:
        assert "constexpr int SKN_WMAX = %d;" % WMAX in f.read()


def test_every_step_lies_in_exactly_one_part_and_wave(facts):
    rows = facts["deal"]
    assert [(r["steps"], r["P"]) for r in rows] == [(s, p) for s in STEPS for p in range(2, 17)]
    for r in rows:
        s, pe = r["steps"], min(r["P"], r["steps"])
        assert r["parts"] == pe, r
        assert r["block_waves"] == min(WMAX, -(-s // pe)), r  # the longest run is part 0's: ceil(S / P_eff) steps
        assert (r["once"], r["end"]) == (s, s), r
        assert (r["out_of_order"], r["empty_parts"], r["uneven"], r["waves_wrong"], r["idle_with_steps"], r["beyond_block"]) == (0,) * 6, r
    assert any(r["parts"] < r["P"] for r in rows) and any(r["parts"] == 1 for r in rows)  # P_eff < P; P_eff < 2: the plain launch


def test_the_grid_names_every_part_and_block_once(facts):
    rows = facts["grid"]
    assert [r["blocks"] for r in rows] == [1, 7, 64]
    for r in rows:
        assert r == dict(blocks=r["blocks"], parts=5, workgroups=5 * r["blocks"], once=5 * r["blocks"], wrong=0), r


def test_every_scratch_float_is_written_exactly_once_inside_the_asked_size(facts):
    rows = facts["scratch"]
    assert len(rows) == 2 * 3 * 3 * 3
    for r in rows:
        assert r["slot"] == r["mb"] * r["bn"] and r["asked"] == r["blocks"] * r["parts"] * r["slot"], r
        assert (r["once"], r["outside"], r["not_contiguous"]) == (r["asked"], 0, 0), r


def test_the_masked_step_of_a_part_is_the_one_that_ends_a_batch_element(facts):
    rows = facts["mask"]
    assert [r["P"] for r in rows] == list(range(2, 10))
    for r in rows:
        assert r == dict(P=r["P"], parts=min(r["P"], 9), steps=9, masked=3, ends=3, wrong=0, masked_if_k_96=0), r


def test_the_refusal_limits(facts):
    tiles, parts, floats = limits()
    want = []
    for blocks, pe, mb, bn in ((64, 2, 16, 16), (tiles, 2, 16, 16), (tiles + 1, 2, 16, 16), (64, parts, 32, 64), (64, parts + 1, 16, 16), (64, 1, 16, 16),
                               (64, 0, 16, 16), (floats // (2 * 32 * 64), 2, 32, 64), (floats // (2 * 32 * 64) + 1, 2, 32, 64), (tiles, parts, 32, 64),
                               (0, 2, 16, 16)):
        n = blocks * pe * mb * bn
        want.append(dict(blocks=blocks, parts=pe, mb=mb, bn=bn, floats=n, ok=int(2 <= pe <= parts and 1 <= blocks <= tiles and n <= floats)))
    assert facts["fits"] == want
    assert [r["ok"] for r in want] == [1, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0]


def test_the_driver_under_asan_and_ubsan(tmp_path):
    """the same driver as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (nothing is loaded into Python)"""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    out = str(tmp_path / "map_asan")
    b = subprocess.run([gxx, "-x", "c++", "-std=c++14", "-O1", "-g", "-I" + CSRC, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", DRIVER, "-o", out], capture_output=True, text=True)
    if b.returncode and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("this compiler has no ASan / UBSan runtime")
    assert b.returncode == 0, b.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([out] + [str(x) for x in limits()], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stdout + r.stderr and "runtime error:" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-4000:]
