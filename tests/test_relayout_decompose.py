"""CPU checks of the RELAYOUT GRID run detection (tpp-mlir_amd/csrc/rt_relayout.h, relayout_decompose), compiled on its own with the
host C++ compiler: the runs it returns cover exactly the recorded items (every block once, whatever their order), two tensors through
one handle are two runs, and groups that are not whole-tensor grids - a hole, a duplicated or displaced block, strided outputs - are
refused (they stay on the item kernel). Which runs get 16-byte accesses follows the bases' and strides' alignment."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
T = 32


@pytest.fixture(scope="module")
def decompose(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not cxx:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("relayout") / "decompose")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC, "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "relayout", "decompose_main.cpp"), "-o", exe])

    def call(op, esz, m, n, ldi, ldo, items):
        text = "%d %d %d %d %d %d %d\n" % (op, esz, m, n, ldi, ldo, len(items)) + "".join("%d %d\n" % it for it in items)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        nr = int(out[0])
        runs = [tuple(int(v) for v in out[1 + k].split()) for k in range(max(nr, 0))]
        return nr, runs

    return call


def expand(runs, esz):
    got = []
    for in0, out0, R, C, ir, ic, orr, oc, _ in runs:
        got += [(in0 + (r * ir + c * ic) * esz, out0 + (r * orr + c * oc) * esz) for r in range(R) for c in range(C)]
    return sorted(got)


def pack_items(A, Ap, R, Cc, esz, perm=False, ldo=T, block=None):
    RB, CB = R // T, Cc // T
    block = T * ldo if block is None else block
    return [(A + (i * T * Cc + j * T) * esz, Ap + ((j * RB + i) if perm else (i * CB + j)) * block * esz) for i in range(RB) for j in range(CB)]


A, W, AP, WP = 1 << 20, 1 << 28, 1 << 32, 3 << 32


@pytest.mark.parametrize("esz,op", [(4, 1), (2, 1), (2, 28)])
@pytest.mark.parametrize("perm", [False, True])
def test_one_tensor_is_one_run_in_any_order(decompose, esz, op, perm):
    items = pack_items(A, AP, 512, 256, esz, perm=perm)
    shuffled = [items[i] for i in np.random.default_rng(0).permutation(len(items))]
    nr, runs = decompose(op, esz, T, T, 256, T, shuffled)
    assert nr == 1 and runs[0][-1] == 1, runs
    assert expand(runs, esz) == sorted(items)
    # the inner index is the one with the smaller source step (consecutive workgroups on neighbouring source rows)
    assert abs(runs[0][5]) <= abs(runs[0][4])


def test_unpack_and_two_tensors_through_one_handle(decompose):
    un = [(AP + (i * 16 + j) * T * T * 4, A + (i * T * 512 + j * T) * 4) for i in range(16) for j in range(16)]
    nr, runs = decompose(1, 4, T, T, T, 512, un)
    assert nr == 1 and expand(runs, 4) == sorted(un)
    two = pack_items(A, AP, 256, 1024, 4) + pack_items(W, WP, 1024, 1024, 4, perm=True)
    nr, runs = decompose(1, 4, T, T, 1024, T, two)
    assert nr == 2 and expand(runs, 4) == sorted(two)


def test_what_is_not_a_whole_tensor_grid_is_refused(decompose):
    items = pack_items(A, AP, 256, 256, 4)
    assert decompose(1, 4, T, T, 256, T, items[:37] + items[38:])[0] == -1  # a hole
    dup = list(items)
    dup[21] = (dup[20][0], dup[21][1])
    assert decompose(1, 4, T, T, 256, T, dup)[0] == -1  # a source block twice, another never
    disp = list(items)
    disp[45] = (disp[45][0], AP + 64 * T * T * 4)
    assert decompose(1, 4, T, T, 256, T, disp)[0] == -1  # an output off the grid
    assert decompose(1, 4, T, T, 256, 40, pack_items(A, AP, 256, 256, 4, ldo=40))[0] == -1  # strided outputs (ldo != n)
    assert decompose(28, 2, 31, T, 256, T, pack_items(A, AP, 256, 256, 2))[0] == -1  # VNNI-2 of an odd row count
    # more than 16 pieces: 17 separate tensors of one block row each
    many = [it for t in range(17) for it in pack_items(A + t * (1 << 22), AP + t * (1 << 22), T, 256, 4)]
    nr, runs = decompose(1, 4, T, T, 256, T, many)
    assert nr == -1


def test_unaligned_bases_keep_the_element_path(decompose):
    items = [(a + 4, o + 4) for a, o in pack_items(A, AP, 256, 256, 4)]
    nr, runs = decompose(1, 4, T, T, 256, T, items)
    assert nr == 1 and runs[0][-1] == 0 and expand(runs, 4) == sorted(items)
    nr, runs = decompose(1, 4, T, 30, 256, 30, pack_items(A, AP, 256, 240, 4, ldo=30))
    assert nr == -1 or runs[0][-1] == 0
