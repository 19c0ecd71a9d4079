"""What the gfx950 code object of tpp-mlir_amd/csrc/brgemm_bf16_dma256_chain.hip holds: a device-only compile with
-Rpass-analysis=kernel-resource-usage, read per kernel. (The single-call kernels' counterparts are dma256_codeobj.py and dma256_edge_codeobj.py.)"""
import os
import re
import shutil
import subprocess
import tempfile

from dma256_codeobj import FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc", "brgemm_bf16_dma256_chain.hip")
# B image -> mangled entry point (rounds are a run-time argument, ChainArgs::groups: one kernel per image)
KERNELS = {0: "_ZN3tpp24brgemm_bf16_dma256_chainENS_9ChainArgsE", 2: "_ZN3tpp30brgemm_bf16_dma256_chain_flatbENS_9ChainArgsE",
           4: "_ZN3tpp30brgemm_bf16_dma256_chain_vnni4ENS_9ChainArgsE"}


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


def launcher_lds_bytes():
    """the dynamic LDS the launcher asks for: its `constexpr size_t lds = <slots> * <bytes>;`"""
    with open(SRC) as f:
        m = re.findall(r"constexpr size_t lds = (\d+) \* (\d+);", f.read())
    assert len(m) == 1, m
    return int(m[0][0]) * int(m[0][1])
