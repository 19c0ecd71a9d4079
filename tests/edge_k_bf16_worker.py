"""Worker of tests/test_edge_k_bf16_gpu.py, and the call helpers the test shares with it. As a program (its own process: strict mode is
chosen before anything is queued, the ragged-k mode comes from the environment): one whole-layer bf16 call with a ragged k under
TPP_HIP_STRICT=1 and TPP_HIP_EDGE_K_BF16=<mode>, three times on the same data. Prints one JSON line: the settings as the library read
them, the kernel each call reported, the counters and a digest of each result's bits.
  edge_k_bf16_worker.py <mode> <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <k> <br> <seed>"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("tpp-mlir_amd")
from edge_tiles_bf16_worker import BF16, VB, b_image, digest  # noqa: E402,F401
from oracle import pyoracle as orc  # noqa: E402


def operands(m, n, k, br, seed, lo=-1.0):
    """bf16 uniform A [m][br k] in [lo, 1), B (br k x n elements in whatever image) in [lo / 2, 0.5), C [m][n], bias [n] (+ 8 guard
    elements each)"""
    rng = np.random.default_rng(seed)
    return [orc.f32_to_bf16(rng.uniform(lo * s, s, cnt + 8).astype(np.float32)) for cnt, s in ((m * k * br, 1), (k * br * n, 0.5), (m * n, 1), (n, 1))]


def layer_call(rt, image, m, n, k, br, A, B, C, D, beta0=False, bias=True, relu=True, force=None):
    """one whole-layer bf16 invoke - br batch elements, each k wide, of a row-major A [m][br k] and of B [br k][n] in image `image` - on
    device copies; returns the whole C buffer after the call (uint16) and what xsmm_hip_last_refined_kernel reported"""
    import torch
    flags = (4 if beta0 else 0) | (VB if image else 0)
    with b_image(rt, image):
        if force is not None:
            rt.force_variant(force)
        try:
            h = rt.fused_brgemm_dispatch(BF16, m, n, k, k * br, n, n, k, k * n, flags, 0, 5 if relu else 0, 4 if bias else 0, 1 if bias else 0)
        finally:
            if force is not None:
                rt.force_variant(-1)
    dA, dB, dC, dD = (torch.from_numpy(x.view(np.int16).copy()).cuda() for x in (A, B, C, D))
    rt.fused_brgemm(BF16, h, dA, 0, dB, 0, dC, 0, dD, 0, br)
    refined = rt.last_refined_kernel()
    return dC.cpu().numpy().view(np.uint16), refined


if __name__ == "__main__":
    mode, image, m, n, k, br, seed = (int(x) for x in sys.argv[1:8])
    rt = pkg.get_runtime()
    out = {"strict": rt.get_strict(), "edge_k_bf16_from_env": rt.set_edge_k_bf16(mode), "kernels": [], "digests": []}
    A, B, C, D = operands(m, n, k, br, seed)
    for _ in range(3):
        got, refined = layer_call(rt, image, m, n, k, br, A, B, C, D)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.edge_k_bf16_stats())
    print(json.dumps(out))
