"""CPU check of the edge-tile maps of the 256x256 bf16 tile (tpp-mlir_amd/csrc/brgemm_bf16_dma256_edge.h, xsmm_hip_set_dma256_edge): the header
the kernel, its launcher and the runtime include, compiled as plain host C++ with tests/dma256_edge_map/driver.cpp. For each output shape
every element of C is stored by exactly one workgroup of the ceil-divided grid, every tile lies inside the matrix, every tile's first
column is a multiple of 8 (16-byte pieces of C, of the B images and of the bias row), and the predicate the kernel's epilogue uses (local
row / column at or behind d256e_skip) is d256e_owns. The control: without the predicate the overlap elements are stored twice."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
SHAPES = [(256, 264), (264, 256), (511, 512), (520, 776), (1000, 504), (4100, 4096)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("dma256_edge_map") / "map")
    subprocess.check_call([cc, "-x", "c++", "-std=c++14", "-O2", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "dma256_edge_map", "driver.cpp"), "-o", out])
    return out


def facts(exe, m, n):
    out = {}
    for l in subprocess.run([exe, str(m), str(n)], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines():
        f = l.split()
        out[f[0]] = f[1:]
    return out


@pytest.mark.parametrize("m,n", SHAPES)
def test_every_element_is_stored_by_exactly_one_workgroup(exe, m, n):
    f = facts(exe, m, n)
    tm, tn = -(-m // 256), -(-n // 256)
    assert f["tiles"] == [str(tm), str(tn)]
    assert f["origins"] == ["outside", "0", "col_off8", "0"], f["origins"]
    assert f["owned"] == ["once", str(m * n), "never", "0", "more", "0", "outside_tile", "0", "skip_mismatch", "0"], f["owned"]


@pytest.mark.parametrize("m,n", SHAPES)
def test_the_control_without_the_predicate_the_overlap_is_stored_twice(exe, m, n):
    f = facts(exe, m, n)["unpredicated"]
    tm, tn = -(-m // 256), -(-n // 256)
    # the shifted last tile row shares 256 tm - m rows with the one in front of it, the last tile column 256 tn - n columns
    orow, ocol = 256 * tm - m, 256 * tn - n
    twice = orow * n + ocol * m - orow * ocol
    assert twice > 0
    assert f == ["twice", str(twice), "never", "0"], f


def test_an_extent_below_the_tile_is_refused(exe):
    for m, n in ((255, 512), (512, 248)):
        assert subprocess.run([exe, str(m), str(n)], capture_output=True).returncode == 3
