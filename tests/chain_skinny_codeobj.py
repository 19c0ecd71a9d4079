"""What the gfx950 code object of tpp-mlir_amd/csrc/brgemm_bf16_skinny_chain.hip holds: a device-only compile with
-Rpass-analysis=kernel-resource-usage, read per kernel. (The unsplit kernel's counterpart is skinny_codeobj.py, whose instance table and
LDS formula hold here too.)"""
import os

import skinny_codeobj
from skinny_codeobj import INSTANCES, ROOT

SRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc", "brgemm_bf16_skinny_chain.hip")


def mangled(img, bn, mb):
    return "_ZN3tpp24brgemm_bf16_skinny_chainILi%dELi%dELi%dEEEvNS_9ChainArgsE" % (img, bn, mb)


KERNELS = {i: mangled(*i) for i in INSTANCES}


def resource_usage():
    """{kernel name: {vgprs, agprs, scratch, sgpr_spill, vgpr_spill, static_lds}} of every kernel in the code object"""
    return skinny_codeobj.resource_usage(SRC)
