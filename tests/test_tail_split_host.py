"""The tail split (xsmm_hip_set_tail_split) without a GPU: the build's own resource report of brgemm_f32_lw.hip - the three tail
instances exist and no instance of the file spills - and the two new entry points of the built library."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f32_loader_wave_kernels_have_tail_instances_and_do_not_spill():
    """a spilling instance still passes every parity test and runs several times slower; the tail instances carry the body path, the
    split epilogue and the run-time test between them, so they are the ones most at risk"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    src = os.path.join(ROOT, "tpp-mlir_amd", "csrc", "brgemm_f32_lw.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", os.path.join(tmp, "k.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) >= 20, (len(names), len(scratch))
    # brgemm_f32_lw<WM, WN, WK, GROUPED, NL, NSLOT, NLB, SPLIT, TAIL>: the instances whose ninth argument is true
    tail = [n for n in names if re.match(r"_ZN3tpp13brgemm_f32_lwI(Li\d+E){3}Lb[01]E(Li\d+E){3}Lb0ELb1EEE", n)]
    assert len(tail) >= 3, names
    bad = [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not bad, "spilling kernels: %s" % bad


def test_library_exports_the_tail_split_entry_points():
    importlib.import_module("tpp-mlir_amd.build").build()
    lib = importlib.import_module("tpp-mlir_amd.runtime").load_library()  # (signatures from runtime.py; no device needed)
    first = lib.xsmm_hip_set_tail_split(1)
    try:
        assert first == 0 or "TPP_HIP_TAIL_SPLIT" in os.environ  # off by default
        assert lib.xsmm_hip_set_tail_split(16) == 1   # returns the previous setting
        assert lib.xsmm_hip_set_tail_split(17) == -1  # refused ...
        assert lib.xsmm_hip_set_tail_split(-1) == -1
        assert lib.xsmm_hip_set_tail_split(0) == 16   # ... and the setting was left alone
        assert lib.xsmm_hip_set_tail_split(2) == 0
        out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
        lib.xsmm_hip_tail_split_stats(out)
        assert all(v >= 0 for v in out)
    finally:
        lib.xsmm_hip_set_tail_split(first if first >= 0 else 0)
