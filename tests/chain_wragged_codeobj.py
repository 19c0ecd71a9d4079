"""The gfx950 code object of tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_wragged.hip as the compiler reports it: one device-only compile with
-Rpass-analysis=kernel-resource-usage. report() returns {kernel symbol: (scratch bytes per lane, VGPRs, AGPRs)}. A plain module of
tests/test_chain_wragged_codeobj.py, not a conftest."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402
from chain_width_rounds_codeobj import parse, symbol as _symbol  # noqa: E402


def symbol(tile, b_kind):
    """brgemm_bf16_lw<tile..., SUP = 1, MULTI = true, b_kind, 11>(ChainArgs)"""
    return _symbol(tile, b_kind, mode=11)


def report():
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([build.hipcc(), "--offload-arch=" + build.ARCH, "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(CSRC, "brgemm_bf16_lw_chain_wragged.hip"),
                            "-o", os.path.join(tmp, "k.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return parse(r.stderr)
