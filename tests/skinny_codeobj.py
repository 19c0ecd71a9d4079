"""What the gfx950 code object of tpp-mlir_amd/csrc/brgemm_bf16_skinny.hip holds: a device-only compile with
-Rpass-analysis=kernel-resource-usage, read per kernel. (The 256x256 edge tiles' counterpart is dma256_edge_codeobj.py.)"""
import os
import re
import shutil
import subprocess
import tempfile

from dma256_codeobj import FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc", "brgemm_bf16_skinny.hip")
# the instance table: B image (0 VNNI-2, 2 flat, 4 VNNI-4) x BN x MB; a flat B has no BN = 16 instance
INSTANCES = [(img, bn, mb) for img in (0, 2, 4) for bn in (16, 32, 64) if not (img == 2 and bn == 16) for mb in (16, 32)]
WMAX = 8


def mangled(img, bn, mb):
    return "_ZN3tpp18brgemm_bf16_skinnyILi%dELi%dELi%dEEEvNS_8GemmArgsE" % (img, bn, mb)


KERNELS = {i: mangled(*i) for i in INSTANCES}


def partial_lds_bytes(bn, mb):
    """the partial accumulators of waves 1 .. WMAX - 1: (MB / 16) x (BN / 16) x 4 floats per lane"""
    return (WMAX - 1) * (mb // 16) * (bn // 16) * 4 * 64 * 4


def resource_usage(src=SRC):
    """{kernel name: {vgprs, agprs, scratch, sgpr_spill, vgpr_spill, static_lds}} of every kernel in the code object of `src` (this file's
    kernel, or the split's or the chain's: the same instance table, LDS formula and limits hold for all three)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "k.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        out[name] = {}
        for f, pat in FIELDS.items():
            m = re.search(pat, b)
            assert m, (name, f)
            out[name][f] = int(m.group(1))
    return out
