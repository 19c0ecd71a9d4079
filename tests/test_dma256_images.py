"""CPU check of the B image maps of the 256x256 bf16 tile (tpp-mlir_amd/csrc/brgemm_bf16_dma256_images.h, xsmm_hip_set_dma256_images): the
header the kernel and its launcher include, compiled as plain host C++ with tests/dma256_images/driver.cpp. For the flat and the VNNI-4
image (and the VNNI-2 image the kernel has always had): the 16 LDS-DMA instructions of a chunk write every byte of the 16 KiB B slot exactly
once, from sources inside the chunk's 32 k-rows and the tile's 256 columns; every fragment read of (wave column, column tile, k-step, lane)
- the transpose reads simulated with the lane map tools/ubench/tr16_probe.hip documents - holds k = 16 ks + 8 lh .. + 7 of column 128 wn +
32 j + li; counted with bank = (a / 4) mod 64 per 32-lane half, equal addresses broadcast, every B fragment read of both new images is
conflict-free, and the same count on the flat image without its swizzle is 4-way.
And, compile-only (tests/dma256_codeobj.py): the gfx950 code object holds exactly the three kernels, without scratch, within 512 registers,
on a 128 KiB ring."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build  # noqa: E402
import dma256_codeobj  # noqa: E402

K0, N0 = 32, 256  # the driver's chunk and column tile


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    try:
        cc = build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    exe = str(tmp_path_factory.mktemp("dma256_images") / "images")
    # C++14: the header is for any host compiler of that standard
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "dma256_images", "driver.cpp"), "-o", exe])
    out = {}
    for l in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = l.split()
        if f[0] in ("cover", "src", "frag", "ways"):
            out[(f[0], int(f[1]), int(f[2]))] = f[3:]
        else:
            out[f[0]] = f[1:]
    return out


IMAGES = [(0, 1), (2, 1), (4, 1), (2, 0)]  # (image, swizzled); the last one is the control


def test_every_case_is_there(facts):
    assert set(facts) == {(w, i, s) for w in ("cover", "src", "frag") for i, s in IMAGES} | {("ways", 2, 1), ("ways", 4, 1), ("ways", 2, 0), "steps", "ldb"}
    # one schedule for all images: 8 KiB from k-step 0 to 1, 2 KiB from a fragment's first read to its second; 16 KiB slots; images 0, 2, 4
    assert facts["steps"] == ["8192", "2048", "slots", "16384", "16384", "ok", "1", "1", "1", "0"]
    # ldb: 16-byte source pieces (flat: % 8, VNNI-4: % 2), lane offsets in 31 bits, at least the tile's columns
    assert facts["ldb"] == ["1", "0", "1", "0", "0", "0"]


@pytest.mark.parametrize("img,swz", IMAGES)
def test_the_dma_writes_every_byte_of_the_slot_once_from_inside_the_chunk(facts, img, swz):
    c = facts[("cover", img, swz)]
    assert c == ["bytes", "16384", "min", "1", "max", "1", "misaligned", "0"], c
    s = facts[("src", img, swz)]
    assert s == ["k", str(K0), str(K0 + 31), "c", str(N0), str(N0 + 255)], s


@pytest.mark.parametrize("img,swz", IMAGES)
def test_every_fragment_read_holds_its_lanes_eight_k_of_its_column(facts, img, swz):
    f = facts[("frag", img, swz)]
    # 2 wave columns x 4 column tiles x 2 k-steps x 2 reads x 64 lanes x 4 elements
    assert f == ["reads", str(2 * 4 * 2 * 2 * 64 * 4), "wrong", "0", "oob", "0", "unaligned", "0"], f


def test_the_fragment_reads_are_conflict_free_and_the_unswizzled_flat_image_is_not(facts):
    assert facts[("ways", 2, 1)] == ["1"] and facts[("ways", 4, 1)] == ["1"]
    assert facts[("ways", 2, 0)] == ["4"], "the control: without the swizzle the four rows of a 16-lane group share their banks"


def test_the_code_object_holds_the_three_kernels_without_scratch():
    k = dma256_codeobj.resource_usage()
    assert sorted(k) == sorted(dma256_codeobj.KERNELS.values()), sorted(k)
    for name, r in k.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["vgprs"] + r["agprs"] <= 512, (name, r)
        assert r["static_lds"] == 0, (name, r)  # the ring is dynamic LDS: the launcher's figure below
    assert dma256_codeobj.launcher_lds_bytes() == 128 * 1024
