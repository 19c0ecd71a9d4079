"""What the gfx950 code object of tpp-mlir_amd/csrc/brgemm_bf16_skinny_chain.hip holds: a device-only compile with
-Rpass-analysis=kernel-resource-usage, read per kernel. (The unsplit kernel's counterpart is skinny_codeobj.py, whose instance table and
LDS formula hold here too.)"""
import os
import re
import shutil
import subprocess
import tempfile

from dma256_codeobj import FIELDS
from skinny_codeobj import INSTANCES, ROOT

SRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc", "brgemm_bf16_skinny_chain.hip")


def mangled(img, bn, mb):
    return "_ZN3tpp24brgemm_bf16_skinny_chainILi%dELi%dELi%dEEEvNS_9ChainArgsE" % (img, bn, mb)


KERNELS = {i: mangled(*i) for i in INSTANCES}


def resource_usage():
    """{kernel name: {vgprs, agprs, scratch, sgpr_spill, vgpr_spill, static_lds}} of every kernel in the code object"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", SRC, "-o", os.path.join(tmp, "k.o"),
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
