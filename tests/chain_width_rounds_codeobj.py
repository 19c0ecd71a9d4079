"""The gfx950 code object of tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_wrounds.hip as the compiler reports it: one device-only compile with
-Rpass-analysis=kernel-resource-usage. report() returns {kernel symbol: (scratch bytes per lane, VGPRs, AGPRs)}. A plain module of
tests/test_chain_width_rounds_launch.py, not a conftest."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

# BLW_TILES (brgemm_bf16_lw_launch.h): WM, WN, WK, TM, TN, NSLOT, NLA, NLB of tiles 0 .. 3
TILES = [(1, 2, 2, 1, 1, 8, 1, 2), (2, 2, 1, 1, 1, 8, 1, 1), (2, 2, 1, 1, 2, 6, 1, 2), (2, 2, 1, 2, 2, 4, 1, 1)]


def symbol(tile, b_kind, mode=10):
    """brgemm_bf16_lw<tile..., SUP = 1, MULTI = true, b_kind, mode>(ChainArgs)"""
    return "_ZN3tpp14brgemm_bf16_lwI" + "".join("Li%dE" % a for a in TILES[tile]) + "Li1ELb1ELi%dELi%dEEEvNS_9ChainArgsE" % (b_kind, mode)


def parse(text):
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", text)]
    agprs = [int(x) for x in re.findall(r"AGPRs: (\d+)", text)]
    assert len(names) == len(scratch) == len(vgprs) == len(agprs) == len(set(names)), (len(names), len(scratch), len(vgprs), len(agprs))
    return {n: (s, v, a) for n, s, v, a in zip(names, scratch, vgprs, agprs)}


def report():
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([build.hipcc(), "--offload-arch=" + build.ARCH, "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(CSRC, "brgemm_bf16_lw_chain_wrounds.hip"),
                            "-o", os.path.join(tmp, "k.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return parse(r.stderr)
