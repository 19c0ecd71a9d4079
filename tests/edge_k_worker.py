"""Worker of tests/test_edge_k_gpu.py, and the call helper the test shares with it. As a program (its own process: strict mode is chosen
before anything is queued, the ragged-k mode comes from the environment): one whole-layer f32 call with a ragged k per forced tile under
TPP_HIP_STRICT=1 and TPP_HIP_EDGE_K=<variant>, three times on the same data. Prints one JSON line: the settings as the library read
them, the kernel each call reported, the counters and a digest of each result's bits.
  edge_k_worker.py <variant> <m> <n> <k> <br> <seed>"""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("tpp-mlir_amd")
F32, BF16 = 1, 2


def operands(m, n, k, br, seed, lda=None, ldb=None, ldc=None, lo=-1.0):
    """uniform [lo, 1) A [m][lda], B [br k][ldb], C [m][ldc], bias [ldb] (+ 8 guard elements each)"""
    rng = np.random.default_rng(seed)
    lda, ldb, ldc = lda or k * br, ldb or n, ldc or n
    return [rng.uniform(lo, 1, s + 8).astype(np.float32) for s in (m * lda, k * br * ldb, m * ldc, ldb)]


def layer_call(rt, m, n, k, br, A, B, C, D, dt=F32, lda=None, ldb=None, ldc=None, beta0=False, bias=True, relu=True, force=None):
    """one whole-layer invoke - br batch elements, each k wide, of row-major operands - on device copies; returns the whole C buffer after
    the call and what xsmm_hip_last_refined_kernel reported"""
    import torch
    lda, ldb, ldc = lda or k * br, ldb or n, ldc or n
    if force is not None:
        rt.force_variant(force)
    try:
        h = rt.fused_brgemm_dispatch(dt, m, n, k, lda, ldb, ldc, k, k * ldb, 4 if beta0 else 0, 0, 5 if relu else 0, 4 if bias else 0, 1 if bias else 0)
    finally:
        if force is not None:
            rt.force_variant(-1)
    dA, dB, dC, dD = (torch.from_numpy(x.copy()).cuda() for x in (A, B, C, D))
    rt.fused_brgemm(dt, h, dA, 0, dB, 0, dC, 0, dD, 0, br)
    refined = rt.last_refined_kernel()
    return dC.cpu().numpy(), refined


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).view(np.uint32).tobytes()).hexdigest()


if __name__ == "__main__":
    variant, m, n, k, br, seed = (int(x) for x in sys.argv[1:7])
    rt = pkg.get_runtime()
    out = {"strict": rt.get_strict(), "edge_k_from_env": rt.set_edge_k(variant), "kernels": [], "digests": []}
    A, B, C, D = operands(m, n, k, br, seed)
    for _ in range(3):
        got, refined = layer_call(rt, m, n, k, br, A, B, C, D)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.edge_k_stats())
    print(json.dumps(out))
