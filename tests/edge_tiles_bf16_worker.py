"""Worker of tests/test_edge_tiles_bf16_gpu.py, and the call helpers the test shares with it. As a program (its own process: strict mode is
chosen before anything is queued, the edge-tile mode comes from the environment): one ragged whole-layer bf16 call under TPP_HIP_STRICT=1
and TPP_HIP_EDGE_TILES=<mode>, three times on the same data. Prints one JSON line: the settings as the library read them, the kernel each
call reported, the counters and a digest of each result's bits.
  edge_tiles_bf16_worker.py <mode> <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <K> <seed>"""
import contextlib
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("tpp-mlir_amd")
from oracle import pyoracle as orc  # noqa: E402

BF16, VB, VC = 2, 2048, 8192


@contextlib.contextmanager
def b_image(rt, image):
    """dispatches inside see a VNNI-`image` B operand (0: flat - the factor stays what it is); the runtime's and the oracle's factor"""
    if not image:
        yield
        return
    old, old_o = rt.set_vnni_factor(image), orc.set_vnni_factor(image)
    try:
        yield
    finally:
        rt.set_vnni_factor(old)
        orc.set_vnni_factor(old_o)


def operands(m, n, K, seed, lda=None, ldb=None, ldc=None):
    """bf16 uniform A [m][lda] in [-1, 1), B (K x ldb elements in whatever image) in [-0.5, 0.5), C [m][ldc], bias [ldb] (+ 8 guard elements each)"""
    rng = np.random.default_rng(seed)
    lda, ldb, ldc = lda or K, ldb or n, ldc or n
    return [orc.f32_to_bf16(rng.uniform(-s, s, cnt + 8).astype(np.float32)) for cnt, s in ((m * lda, 1), (K * ldb, 0.5), (m * ldc, 1), (ldb, 1))]


def layer_call(rt, image, m, n, K, A, B, C, D, k=64, lda=None, ldb=None, ldc=None, beta0=False, bias=True, relu=True, offs=(0, 0, 0, 0), force=None,
               vnni_c=False):
    """one whole-layer bf16 invoke (k-wide batch elements of a row-major A, B in image `image`) on device copies; returns the whole C buffer
    after the call (uint16) and what xsmm_hip_last_refined_kernel reported"""
    import torch
    lda, ldb, ldc = lda or K, ldb or n, ldc or n
    flags = (4 if beta0 else 0) | (VB if image else 0) | (VC if vnni_c else 0)
    with b_image(rt, image):
        if force is not None:
            rt.force_variant(force)
        try:
            h = rt.fused_brgemm_dispatch(BF16, m, n, k, lda, ldb, ldc, k, k * ldb, flags, 0, 5 if relu else 0, 4 if bias else 0, 1 if bias else 0)
        finally:
            if force is not None:
                rt.force_variant(-1)
    dA, dB, dC, dD = (torch.from_numpy(x.view(np.int16).copy()).cuda() for x in (A, B, C, D))
    rt.fused_brgemm(BF16, h, dA, offs[0], dB, offs[1], dC, offs[2], dD, offs[3], K // k)
    refined = rt.last_refined_kernel()
    return dC.cpu().numpy().view(np.uint16), refined


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).view(np.uint16).tobytes()).hexdigest()


if __name__ == "__main__":
    mode, image, m, n, K, seed = (int(x) for x in sys.argv[1:7])
    rt = pkg.get_runtime()
    out = {"strict": rt.get_strict(), "edge_tiles_from_env": rt.set_edge_tiles(mode), "kernels": [], "digests": []}
    A, B, C, D = operands(m, n, K, seed)
    for _ in range(3):
        got, refined = layer_call(rt, image, m, n, K, A, B, C, D)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.edge_tiles_stats())
    print(json.dumps(out))
