"""CPU check of the maps of the skinny-batch bf16 kernel (tpp-mlir_amd/csrc/brgemm_bf16_skinny.h, xsmm_hip_set_skinny_bf16): the header the
kernel, its launcher and the planner include, compiled as plain host C++ with tests/skinny_map/driver.cpp. For each of the eight B instances
(VNNI-2 and VNNI-4 at BN 16, 32, 64; flat at 32, 64):
  - every (k, column) of a step's 32 x BN slab is loaded exactly once, at the byte offset the image gives that element;
  - element e of the operand of MFMA j of lane l is k = 8 (l >> 4) + e of column c (l & 15) + j - and with the selection of another image it
    is not (the control);
  - for m in {1, 7, 16, 17, 31} and n in {16, 24, 72, 200, 1000} (n >= BN) every (row < m, column < n) is stored exactly once, every block
    and every load origin lies inside the operand at a multiple of 8 columns, the predicate the kernel uses is skn_owns - and without the
    predicate the overlap of a shifted last block is stored twice (the control);
  - the masks for k mod 32 in {0, 8, 16, 24} keep exactly the k below the limit, and never mask a whole step;
  - every step belongs to exactly one wave, in order, for steps in {1, 2, 3, W - 1, W, W + 1, 5 W + 3}.
The same driver runs once more as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "skinny_map", "driver.cpp")
INSTANCES = [(img, bn) for img in (0, 2, 4) for bn in (16, 32, 64) if not (img == 2 and bn == 16)]
VFAC = {0: 2, 2: 1, 4: 4}
MS, NS = (1, 7, 16, 17, 31), (16, 24, 72, 200, 1000)
WMAX = 8


def compiler():
    return shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("skinny_map") / "map")
    subprocess.check_call([compiler(), "-x", "c++", "-std=c++14", "-O2", "-Wall", "-I" + CSRC, DRIVER, "-o", out])
    return out


def facts(exe, img, bn):
    """{first word: [fields of every such line as a {name: int} dict]}"""
    out = {}
    for l in subprocess.run([exe, str(img), str(bn)], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = l.split()
        out.setdefault(f[0], []).append({f[i]: int(f[i + 1]) for i in range(1, len(f) - 1, 2)})
    return out


def test_the_wave_limit_restated_here_is_the_headers():
    with open(os.path.join(CSRC, "brgemm_bf16_skinny.h")) as f:
        assert "constexpr int SKN_WMAX = %d;" % WMAX in f.read()


@pytest.mark.parametrize("img,bn", INSTANCES)
def test_every_element_of_a_steps_slab_is_loaded_exactly_once(exe, img, bn):
    f = facts(exe, img, bn)
    assert f["instance"] == [dict(image=img, bn=bn, c=bn // 16, rows=8 // VFAC[img], dwords=bn // 16 * VFAC[img] // 2)]
    assert f["slab"] == [dict(once=32 * bn, never=0, more=0, outside=0, byte_mismatch=0)]


@pytest.mark.parametrize("img,bn", INSTANCES)
def test_fragment_j_holds_its_columns_eight_k_values_and_the_wrong_images_selection_is_caught(exe, img, bn):
    rows = {r["selection_of"]: r for r in facts(exe, img, bn)["frag"]}
    assert sorted(rows) == [0, 2, 4]
    assert rows[img] == dict(selection_of=img, wrong=0, off_lane=0)
    for other in (0, 2, 4):
        if other != img:
            assert rows[other]["wrong"] + rows[other]["off_lane"] > 0, (img, bn, other)


@pytest.mark.parametrize("img,bn", INSTANCES)
def test_every_output_is_stored_exactly_once_and_without_the_predicate_twice(exe, img, bn):
    rows = facts(exe, img, bn)["store"]
    assert [(r["m"], r["n"]) for r in rows] == [(m, n) for m in MS for n in NS if n >= bn]
    ragged = 0
    for r in rows:
        m, n = r["m"], r["n"]
        blocks = -(-n // bn)
        assert r["blocks"] == blocks
        assert (r["once"], r["never"], r["more"]) == (m * n, 0, 0), r
        assert (r["outside"], r["origin_off8"], r["pred_mismatch"], r["split_lane"], r["unpredicated_never"]) == (0, 0, 0, 0, 0), r
        # the control: the shifted last block shares bn * blocks - n columns with the one in front of it
        assert r["unpredicated_twice"] == (bn * blocks - n) * m, r
        ragged += r["unpredicated_twice"] > 0
    assert ragged >= 5


@pytest.mark.parametrize("img,bn", INSTANCES)
def test_the_ragged_k_masks_keep_exactly_the_k_below_the_limit(exe, img, bn):
    rows = facts(exe, img, bn)["mask"]
    assert [r["kmod"] for r in rows] == [0, 8, 16, 24]
    for r in rows:
        kmod = r["kmod"]
        assert r["steps"] == (2 if kmod == 0 else 3) and r["last_klim"] == (kmod or 32)
        assert (r["kept_below"], r["kept_beyond"], r["dropped_below"], r["full_steps_masked"]) == (kmod or 32, 0, 0, 0), r


@pytest.mark.parametrize("img,bn", INSTANCES[:1])
def test_every_step_belongs_to_exactly_one_wave(exe, img, bn):
    rows = facts(exe, img, bn)["deal"]
    assert [r["steps"] for r in rows] == [1, 2, 3, WMAX - 1, WMAX, WMAX + 1, 5 * WMAX + 3]
    for r in rows:
        assert r == dict(steps=r["steps"], waves=min(WMAX, r["steps"]), once=r["steps"], out_of_order=0, idle=0, end=r["steps"]), r


def test_an_instance_that_does_not_exist_is_refused(exe):
    for img, bn in ((2, 16), (0, 8), (0, 128), (1, 32)):
        assert subprocess.run([exe, str(img), str(bn)], capture_output=True).returncode == 3


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
    for img, bn in INSTANCES:
        r = subprocess.run([out, str(img), str(bn)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0 and "AddressSanitizer" not in r.stdout + r.stderr and "runtime error:" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-4000:]
