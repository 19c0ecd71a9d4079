"""The single-call launch decision (tpp-mlir_amd/csrc/gemm_plan.cpp plan_gemm, plan_gemm_call; carried out by brgemm_f32.hip launch_gemm) on a
CPU under every set of the eight mode switches - xsmm_hip_set_dma256_edge, _edge_tiles, _edge_k, _edge_k_bf16, _edge_k8_bf16, _dma256_images,
_tail_split, _f32_halves - with xsmm_hip_force_split as part of the context. tests/gemm_call_switches/driver.cpp is plain host C++ linked with
the unchanged gemm_plan.cpp. The lattice: f32 and bf16 with a VNNI-2, flat and VNNI-4 B x 13 m x 11 n x 12 k at one and thirteen batch
elements, and a sub-lattice (4 m x 7 n x 4 k, n = 70 and 260 included: n % 4, n % 8) under batch counts 0, 2 and 16, beta 0 / 1 with and
without a bias, a VNNI C, forced variants and the forced generic kernel, each misalignment of GemmAlign, wide and off-grid leading dimensions.
All 256 switch sets in four contexts - "rule" (every member at its rule value, the edge tiles at 2), "eligible" (mode 2 where it exists,
tail_split 2), and two "forcing" ones (tile-naming values, one with a bf16 and one with an f32 tile in edge_tiles; forced split 4) - at 64, 256
and 304 compute units, strict off and on: about 30 million decisions a process, 5 s.

  a  dispatch reads no single-call switch: plan_gemm gives the same variant under every set (handles are cached across mode changes).
  b  one precedence list - dma256 edge, bf16 edge tiles, bf16 ragged k, half-step ragged k, dma256 images, f32 edge tiles, f32 ragged k, tail
     split, halves - and the documented read sets: the first refinement that takes the call under ITS OWN read set wins, P(S) is that launch
     field by field, and P({}) where none does. The two bf16 ragged-k switches never read each other; no bf16-only switch changes an f32 call,
     nor the reverse.
  c  per launch, from the kernels' contracts: at most one of edge / edge_k / edge_k8, each ragged form's k, m >= BM, n >= BN, n % 8 (bf16) /
     n % 4 (f32), a tile that does not divide m and n only with that type's edge tiles on, the 256x256 forms' shapes and images, pointers,
     leading dimensions and strides on the 16-byte grid, halves on tile 1 with split 1 and no tail, a tail only with split 1, a text that
     says what the launch is; strict mode changes nothing but split, tail split and halves. A forced variant, the forced generic kernel, a
     VNNI C and an empty batch get none of the seven refinements that leave the dispatched kernel. (Documented, not a deviation: split, tail
     split and halves act on the K-split f32 tile a call was DISPATCHED on, forced or not - gemm_plan.cpp choose_f32_halves, the forced
     tiles of tests/test_f32_halves_gpu.py and tests/test_tail_split_gpu.py - and halves keeps an empty batch, as launch_f32_lw does.)
  d  planner within launcher: every loader-wave bf16 launch passes blw_launch_ok and has its instance, every 256x256 launch the predicates of
     brgemm_bf16_dma256_edge.h / _images.h and the launchers' own lines, every f32 form the terms of brgemm_f32_lw.hip (restated in the driver,
     lines cited). Planner-accepted, launcher-refused cases print as REFUSED lines: there are none, so the GPU test has no fallback row.
  e  the refusal cascade of launch_gemm: from every refined P(S), zero the mode launch_gemm would zero and plan again - every refinement met
     on the way belongs to a strictly later block (dma256 edge, dma256 images, half-step k, bf16 ragged k, f32 ragged k, edge tiles, split,
     tail split, halves) and the walk ends without a refinement flag within nine steps.
  f  tests/golden/gemm_call_switches.txt: per descriptor and call of a reviewed list, P({}), the eight P({x}) and P(all) in "rule",
     "eligible" and "forcing" (and under xsmm_hip_force_split(2) where it matters), one row per group of compute-unit counts that agree. A
     rule change shows as a diff of that file. Regenerate: build as the `driver` fixture does, then `driver table > tests/golden/gemm_call_switches.txt`.
     The rows of tests/test_call_switches_gpu.py (tests/call_switches_worker.py ROWS) are in it, the same at 64, 256 and 304 compute units.
  g  the driver once more as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (nothing is loaded into Python).
No check found a deviation: the planner is unchanged and this file has no regression case of its own. What the checks catch was tried on
scratch copies of gemm_plan.cpp: the half-step block reading the other ragged-k switch's tile (b), the 256x256 edge block gated on
edge_k_bf16 (b and e), a tail split gated on halves (b), f32 ragged k on a ragged tile without the edge tiles, bf16 edge tiles without
n % 8 or without the C alignment, f32 edge tiles without n % 4 (c and d), dma256 images of a forced variant (c)."""
import difflib
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "gemm_call_switches", "driver.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_call_switches.txt")
HIP_INCLUDE = "/opt/rocm/include"
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build  # noqa: E402
import call_switches_worker as csw  # noqa: E402

RUNS = [(cus, strict) for cus in (64, 256, 304) for strict in (0, 1)]
RUN_TIMEOUT = 600   # seconds per driver process; a sweep takes about 5 here
REFINEMENTS = ["dma256_edge", "bf16_edge_tiles", "bf16_ragged_k", "half_step_k", "dma256_images", "f32_edge_tiles", "f32_ragged_k", "tail_split", "halves"]


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_") and k != "LD_PRELOAD"}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    d = tmp_path_factory.mktemp("gemm_call_switches")
    objs = []
    for src, name in ((os.path.join(CSRC, "gemm_plan.cpp"), "gemm_plan.o"), (DRIVER, "driver.o")):
        obj = str(d / name)
        subprocess.check_call([cc] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(d / "call_switches")
    subprocess.check_call([cc, "--offload-arch=" + build.ARCH] + objs + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def sweeps(driver):
    """the six sweep processes side by side: (exit code, stdout) per (compute units, strict)"""
    procs = {r: subprocess.Popen([driver, "sweep", str(r[0]), str(r[1])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=clean_env())
             for r in RUNS}
    out = {}
    try:
        for r, p in procs.items():
            text, _ = p.communicate(timeout=RUN_TIMEOUT)
            out[r] = (p.returncode, text)
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    return out


@pytest.fixture(scope="module")
def table(driver):
    return subprocess.run([driver, "table"], capture_output=True, text=True, check=True, timeout=RUN_TIMEOUT, env=clean_env()).stdout


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("cus,strict", RUNS)
def test_every_switch_set_keeps_the_precedence_the_invariants_the_launchers_and_the_cascade(sweeps, cus, strict):
    rc, out = sweeps[(cus, strict)]
    print(out[-3000:])
    fails = [l for l in out.splitlines() if l.startswith("FAIL")]
    assert not fails, "\n".join(fails[:20])
    assert rc == 0 and out.strip().endswith("OK"), out[-3000:]
    m = re.search(r"^%d compute units, strict %d: (\d+) descriptors, (\d+) decisions, 0 FAIL$" % (cus, strict), out, re.M)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) > 20000000, out[-500:]
    # d: nothing the planner accepts is refused by its launcher
    assert "planner accepts, launcher refuses: 0" in out and not [l for l in out.splitlines() if l.startswith("REFUSED")]
    # each of the nine refinements at least once per B image it has (the driver asserts it too: FAIL coverage)
    line = [l for l in out.splitlines() if l.startswith("refinements reached:")][0].split(":", 1)[1].split()
    seen = dict(zip(line[0::2], line[1::2]))
    assert list(seen) == REFINEMENTS, seen
    for name, counts in seen.items():
        n = [int(c) for c in counts.split("/")]
        assert len(n) == (1 if name in REFINEMENTS[5:] else 3), (name, counts)
        # (the VNNI-2 image of the 256x256 tile is the dispatched kernel itself: xsmm_hip_set_dma256_images has the flat and the VNNI-4 image)
        assert all(c > 0 for c in (n[1:] if name == "dma256_images" else n)), (name, counts)


def test_decision_table_matches_the_golden_file(table):
    with open(GOLDEN) as f:
        want = f.read()
    if table != want:
        diff = "".join(list(difflib.unified_diff(want.splitlines(True), table.splitlines(True), "golden", "planner"))[:60])
        pytest.fail("the single-call decisions differ from tests/golden/gemm_call_switches.txt:\n" + diff[:12000])
    assert 300 < len(want.splitlines()) < 500


def launches(line):
    """a table row -> (label, context, compute units, {"{}" / switch / "all": launch})"""
    f = line.split(" | ")
    ctx, cus = f[3].split(" cus")
    d = {}
    for cell in f[4:]:
        key, launch = cell.split(" ", 1)
        d[key] = launch
    off = d["{}"]
    return f[0], ctx, cus, {k: off if v == "-" else v for k, v in d.items()}


def winner_of(launch):
    """the switch whose counter a launch moves (tests/call_switches_worker.py SWITCHES), and its text"""
    text = re.search(r'"(.*)"$', launch).group(1)
    head = launch[:launch.index('"')].split()
    if head[0] == "bf16_fast" and "edge" in head:
        return "dma256_edge", text
    if head[0] == "bf16_fast" and head[3] != "b0":
        return "dma256_images", text
    if head[0] == "bf16_lw" and ("edge_k8" in head or "edge_k" in head or "edge" in head):
        return ("edge_k8_bf16" if "edge_k8" in head else "edge_k_bf16" if "edge_k" in head else "edge_tiles"), text
    if head[0] == "f32_lw" and ("edge_k" in head or "edge" in head):
        return ("edge_k" if "edge_k" in head else "edge_tiles"), text
    if any(h.startswith("tail") for h in head):
        return "tail_split", text
    if "halves" in head:
        return "f32_halves", text
    return None, text


def test_the_gpu_rows_are_golden_rows_that_no_compute_unit_count_changes():
    """what tests/test_call_switches_gpu.py hard-codes per row and context is the golden P(all), identical at 64, 256 and 304 compute units
    (the tail-split row, whose shape comes from the device: the row of 256 compute units)"""
    with open(GOLDEN) as f:
        rows = [launches(l) for l in f.read().splitlines() if not l.startswith("#")]
    checked = set()
    for r in csw.ROWS:
        for ctx in ("rule", "eligible"):
            name = ctx + "-split2" if r["split"] == 2 else ctx
            got = [x for x in rows if x[0] == r["golden"] and x[1] == name and ("256" in x[2].split(","))]
            assert len(got) == 1, (r["label"], name, got)
            if r["n"] is not None:
                assert got[0][2] == "64,256,304", (r["label"], name, got[0][2])
            assert winner_of(got[0][3]["all"]) == tuple(r["expect"][ctx]), (r["label"], name, got[0][3]["all"])
            # with the winner's read set alone the launch is the same: the single-switch cells where the read set is one switch
            w = r["expect"][ctx][0]
            if w is not None and len(csw.READS[w]) == 1:
                assert got[0][3]["halves" if w == "f32_halves" else w] == got[0][3]["all"], (r["label"], name)
            checked.add(r["expect"][ctx])
    assert len(csw.ROWS) >= 40 and {w for w, _ in checked} == set(csw.SWITCHES) | {None}
    assert {r["label"] for r in csw.ROWS if r["n"] is not None} == {x[0] for x in rows if x[0].startswith("gpu:")}


@pytest.mark.timeout(1800)
def test_driver_under_asan_and_ubsan(tmp_path):
    """the same driver and the unchanged gemm_plan.cpp as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: the table,
    and the sweep over an eighth of the shape lattice and the whole sub-lattice"""
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "driver_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE, "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", os.path.join(CSRC, "gemm_plan.cpp"), DRIVER, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("this compiler has no ASan / UBSan runtime")
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(clean_env(), ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for args in (["table"], ["sweep", "304", "1", "quick"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=RUN_TIMEOUT)
        assert "AddressSanitizer" not in r.stdout + r.stderr and "runtime error:" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-6000:]
        assert r.returncode == 0 and not [l for l in r.stdout.splitlines() if l.startswith("FAIL")], (r.stdout[-3000:], r.stderr[-3000:])
        if args[0] == "table":
            with open(GOLDEN) as f:
                assert r.stdout == f.read()
        else:
            assert r.stdout.strip().endswith("OK")
