"""Worker of tests/test_chain_dma256_gpu.py, and the helpers the test shares with it. As a program (its own process: strict mode is chosen
before anything is queued; the switch comes from the environment): one bf16 layer chain under TPP_HIP_STRICT=1 and TPP_HIP_CHAIN_DMA256=<mode>
through xsmm_hip_fused_brgemm_chain_invoke. Prints one JSON line: the settings as the library read them, whether the chain ran as one launch,
the counters and a digest of every layer's bits.
  chain_dma256_worker.py <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <k0> <br0> <forced variant at dispatch, -1 none> <seed>"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("tpp-mlir_amd")
from chain_edge_worker import BF16, GUARD_ROWS, VB, RaggedChain, b_image, dev, digest  # noqa: E402

KIND = {2: 0, 0: 2, 4: 4}  # RaggedChain's image (the VNNI factor, 0 flat) -> the B image as the library counts it
V_DMA256 = 18              # GemmVariant of the 256x256 tile (xsmm_hip_force_variant)


def make_chain(rt, image, m, n, k0, br0, seed, layers=3, exact=False, force=None):
    """`layers` layers with bias + relu: layer 0 reads br0 batch elements of k0 columns (stride_a along k), the later layers k = n"""
    return RaggedChain(rt, image, m, n, [k0] + [n] * (layers - 1), [br0] + [1] * (layers - 1), seed, exact=exact, force=force)


def layer0_on_the_tile(rt, ch, dx=None):
    """Layer 0 of `ch` as the 256x256 tile computes it in a single call. The library reaches the divisible kernel only with k % 64 == 0, and
    every k0 of the test is 32 mod 64 - so the call is made on m + 8 rows (8 rows of zeros behind the chain's input) under
    xsmm_hip_set_dma256_edge(2): the first m / 256 tile rows of that launch are unshifted whole tiles of the same kernel text, and an
    output element is one chain over k in k order wherever its tile lies. Returns the m x n result as a host array [m][n]."""
    import torch
    m2, K = ch.m + 8, ch.ks[0] * ch.brs[0]
    x = torch.zeros((m2 + GUARD_ROWS) * ch.ld_in[0], dtype=torch.int16, device="cuda")
    x[:ch.m * ch.ld_in[0]] = (ch.dx if dx is None else dx)[:ch.m * ch.ld_in[0]]
    out = torch.zeros((m2 + GUARD_ROWS) * ch.ldc, dtype=torch.int16, device="cuda")
    with b_image(rt, ch.image):
        h = rt.fused_brgemm_dispatch(BF16, m2, ch.n, ch.ks[0], ch.ld_in[0], ch.ldb, ch.ldc, ch.ks[0], ch.ks[0] * ch.ldb, 4 | (VB if ch.image else 0), 0, 5, 4, 1)
    old = rt.set_dma256_edge(2)
    try:
        before = rt.dma256_edge_stats()
        rt.fused_brgemm(BF16, h, x, 0, ch.dW[0], 0, out, 0, ch.db[0], 0, ch.brs[0])
        rt.synchronize()
        after = rt.dma256_edge_stats()
        assert after[0] == before[0] + 1 and after[3] == KIND[ch.image], (before, after)
    finally:
        rt.set_dma256_edge(old)
    assert K <= ch.ld_in[0]
    return out.cpu().numpy().view(np.uint16).reshape(m2 + GUARD_ROWS, ch.ldc)[:ch.m, :ch.n].copy()


def separate_calls_on_the_tile(rt, ch, dx=None):
    """the chain's calls one by one with the switch off, every one on the 256x256 tile: layer 0 by layer0_on_the_tile when its k is not in
    64-k chunks, the others pinned there - VNNI-2 by the variant forced at dispatch (ch was made with force = V_DMA256), flat and VNNI-4 by
    xsmm_hip_set_dma256_images(2). Returns every layer's host array."""
    rt.set_chain_dma256(0)
    outs = ch.outputs()
    first = 0
    if ch.ks[0] % 64:
        o0 = ch.out_template.copy().reshape(ch.m + GUARD_ROWS, ch.ldc)
        o0[:ch.m, :ch.n] = layer0_on_the_tile(rt, ch, dx)
        outs[0].copy_(dev(o0.reshape(-1)))
        first = 1
    old = rt.set_dma256_images(2 if ch.image != 2 else 0)
    try:
        before = rt.dma256_images_stats()
        for c in ch.calls(outs, dx)[first:]:
            assert rt.kernel_name(c[0]).startswith("brgemm_bf16_dma<256x256>") or ch.image != 2, rt.kernel_name(c[0])
            rt.fused_brgemm(BF16, *c)
        got = ch.host(outs)
        if ch.image != 2:
            assert rt.dma256_images_stats()[0] == before[0] + ch.L - first, "a call did not run on the 256x256 tile"
    finally:
        rt.set_dma256_images(old)
    return got


if __name__ == "__main__":
    image, m, n, k0, br0, force, seed = (int(x) for x in sys.argv[1:8])
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    mode = rt.set_chain_dma256(0)
    out = {"strict": rt.get_strict(), "mode_from_env": mode}
    ch = make_chain(rt, image, m, n, k0, br0, seed, force=None if force < 0 else force)
    rt.set_chain_dma256(mode)
    outs = ch.outputs()
    out["ran_as_one"] = bool(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
    got = ch.host(outs)
    ch.check_windows(got)
    out["digests"] = [digest(g) for g in got]
    out["chain_dma256_stats"] = list(rt.chain_dma256_stats())
    rt.set_chain_dma256(0), rt.set_async(was_async)
    print(json.dumps(out))
