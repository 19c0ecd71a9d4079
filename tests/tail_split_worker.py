"""Worker of tests/test_tail_split_gpu.py (its own process: strict mode is chosen before anything is queued, the tail split comes from
the environment). One whole-layer f32 call with a partial last round of tiles, three times on the same data under TPP_HIP_STRICT=1 and
TPP_HIP_TAIL_SPLIT=1. Prints one JSON line: the settings as the library read them, the kernel each call reported, the counters and a
digest of each result's bits.
  tail_split_worker.py <forced variant> <m> <n> <K> <seed>"""
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


def operands(m, n, K, seed):
    """shared with the test: uniform [-1, 1) A [m][K], B [K][n], C [m][n], bias [n]"""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, s).astype(np.float32) for s in (m * K, K * n, m * n, n)]


def layer_call(rt, variant, m, n, K, A, B, C, D, beta0=False, bias=True, relu=True):
    """one whole-layer invoke (64-k batch elements of row-major operands) of a forced tile variant on device copies; returns C's bits
    after the call and what xsmm_hip_last_refined_kernel reported"""
    import torch
    flags = 4 if beta0 else 0
    rt.force_variant(variant)
    try:
        h = rt.fused_brgemm_dispatch(F32, m, n, 64, K, n, n, 64, 64 * n, flags, 0, 5 if relu else 0, 4 if bias else 0, 1 if bias else 0)
    finally:
        rt.force_variant(-1)
    dA, dB, dC, dD = (torch.from_numpy(x.copy()).cuda() for x in (A, B, C, D))
    rt.fused_brgemm(F32, h, dA, 0, dB, 0, dC, 0, dD, 0, K // 64)
    refined = rt.last_refined_kernel()
    return dC.cpu().numpy(), refined


if __name__ == "__main__":
    variant, m, n, K, seed = (int(x) for x in sys.argv[1:6])
    rt = pkg.get_runtime()
    out = {"strict": rt.get_strict(), "tail_split_from_env": rt.set_tail_split(1), "kernels": [], "digests": []}
    A, B, C, D = operands(m, n, K, seed)
    for _ in range(3):
        got, refined = layer_call(rt, variant, m, n, K, A, B, C, D)
        out["kernels"].append(refined)
        out["digests"].append(hashlib.sha256(got.view(np.uint32).tobytes()).hexdigest())
    out["stats"] = list(rt.tail_split_stats())
    print(json.dumps(out))
