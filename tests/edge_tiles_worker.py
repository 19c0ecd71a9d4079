"""Worker of tests/test_edge_tiles_gpu.py, and the call helper the test shares with it. As a program (its own process: strict mode is
chosen before anything is queued, the edge-tile mode comes from the environment): one ragged whole-layer f32 call per forced tile under
TPP_HIP_STRICT=1 and TPP_HIP_EDGE_TILES=<variant>, three times on the same data. Prints one JSON line per run: the settings as the
library read them, the kernel each call reported, the counters and a digest of each result's bits.
  edge_tiles_worker.py <variant> <m> <n> <K> <seed>"""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("tpp-mlir_amd")
F32 = 1


def operands(m, n, K, seed, lda=None, ldb=None, ldc=None):
    """uniform [-1, 1) A [m][lda], B [K][ldb], C [m][ldc], bias [ldb] (+ 8 guard elements each)"""
    rng = np.random.default_rng(seed)
    lda, ldb, ldc = lda or K, ldb or n, ldc or n
    return [rng.uniform(-1, 1, s + 8).astype(np.float32) for s in (m * lda, K * ldb, m * ldc, ldb)]


def layer_call(rt, m, n, K, A, B, C, D, k=64, lda=None, ldb=None, ldc=None, beta0=False, bias=True, relu=True, offs=(0, 0, 0, 0), force=None):
    """one whole-layer invoke (k-wide batch elements of row-major operands) on device copies; returns the whole C buffer after the call
    and what xsmm_hip_last_refined_kernel reported"""
    import torch
    lda, ldb, ldc = lda or K, ldb or n, ldc or n
    flags = 4 if beta0 else 0
    if force is not None:
        rt.force_variant(force)
    try:
        h = rt.fused_brgemm_dispatch(F32, m, n, k, lda, ldb, ldc, k, k * ldb, flags, 0, 5 if relu else 0, 4 if bias else 0, 1 if bias else 0)
    finally:
        if force is not None:
            rt.force_variant(-1)
    dA, dB, dC, dD = (torch.from_numpy(x.copy()).cuda() for x in (A, B, C, D))
    rt.fused_brgemm(F32, h, dA, offs[0], dB, offs[1], dC, offs[2], dD, offs[3], K // k)
    refined = rt.last_refined_kernel()
    return dC.cpu().numpy(), refined


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).view(np.uint32).tobytes()).hexdigest()


if __name__ == "__main__":
    variant, m, n, K, seed = (int(x) for x in sys.argv[1:6])
    rt = pkg.get_runtime()
    out = {"strict": rt.get_strict(), "edge_tiles_from_env": rt.set_edge_tiles(variant), "kernels": [], "digests": []}
    A, B, C, D = operands(m, n, K, seed)
    for _ in range(3):
        got, refined = layer_call(rt, m, n, K, A, B, C, D)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.edge_tiles_stats())
    print(json.dumps(out))
