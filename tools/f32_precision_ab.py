#!/usr/bin/env python3
"""A/B of the f32 GEMM arithmetic (xsmm_hip_set_f32_precision: exact f32 MFMA against the bf16x6 split) on whole
problems: C2, C3, 4096^3 and the f32 whole-layer rows of tools/refbench.py (k = 64 chunks, br = K / 64). Each case is dispatched in both
modes (the split tile forced in bf16x6 mode) and invoked -n times per mode; the kernel averages come from the profiler around it:
    rocprofv3 --kernel-trace --stats -d <dir> -o ab -- python tools/f32_precision_ab.py -n 50
Printed per case and mode: the kernel name, the mean wall time per invoke (torch events) and the worst relative error against an fp64
truth over the non-cancelled elements (|truth| >= 1 % of its maximum), uniform [-1, 1) inputs."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32 = 1

# name, m, n, K, beta0, bias + relu, the split tile forced in bf16x6 mode (xsmm_hip_force_variant: 12 64x64, 13 64x32 + K2,
# 14 32x32 + K4, 15 128x64 - the output tile of the exact plan: the planner does not put bf16x6 descriptors on the split kernel by itself)
CASES = [
    ("C2 1024x1024x1024 br16", 1024, 1024, 1024, False, False, 12),
    ("C3 512x1024x1024 bias relu", 512, 1024, 1024, True, True, 13),
    ("4096x4096x4096", 4096, 4096, 4096, True, False, 15),
    ("whole 1024x2560x1024", 1024, 2560, 1024, True, False, 12),
    ("whole 1024x1024x512", 1024, 1024, 512, True, False, 12),
    ("whole 256x1024x4096", 256, 1024, 4096, True, False, 14),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=50)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    print("# %-30s %-6s %-32s %10s %12s" % ("case", "mode", "kernel", "us/invoke", "max rel err"))
    for name, m, n, K, beta0, br_relu, tile in CASES:
        if args.only and args.only not in name:
            continue
        A = rng.uniform(-1, 1, m * K).astype(np.float32)
        B = rng.uniform(-1, 1, K * n).astype(np.float32)
        bias = rng.uniform(-1, 1, n).astype(np.float32)
        C = rng.uniform(-1, 1, m * n).astype(np.float32)
        t = A.astype(np.float64).reshape(m, K) @ B.astype(np.float64).reshape(K, n)
        if not beta0:
            t += C.astype(np.float64).reshape(m, n)
        if br_relu:
            t = np.maximum(t + bias.astype(np.float64), 0.0)
        big = np.abs(t) >= 1e-2 * np.abs(t).max()
        dA, dB, dD = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), torch.from_numpy(bias).cuda()
        for mode in (0, 6):
            rt.set_f32_precision(mode)
            rt.force_variant(tile if mode else -1)
            flags = 4 if beta0 else 0
            if br_relu:
                h = rt.fused_brgemm_dispatch(F32, m, n, 64, K, n, n, 64, 64 * n, flags, 0, 5, 4, 1)
            else:
                h = rt.brgemm_dispatch(F32, m, n, 64, K, n, n, 64, 64 * n, flags)
            rt.set_f32_precision(0)
            rt.force_variant(-1)
            dC = torch.from_numpy(C).cuda()

            def run():
                if br_relu:
                    rt.fused_brgemm(F32, h, dA, 0, dB, 0, dC, 0, dD, 0, K // 64)
                else:
                    rt.brgemm(F32, h, dA, 0, dB, 0, dC, 0, K // 64)
            run()
            torch.cuda.synchronize()
            got = dC.cpu().numpy().astype(np.float64).reshape(m, n)
            rel = float((np.abs(got - t)[big] / np.abs(t[big])).max())
            run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.n):
                run()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.n
            print("  %-30s %-6s %-32s %10.2f %12.3g" % (name, "bf16x6" if mode else "exact", rt.kernel_name(h), us, rel), flush=True)


if __name__ == "__main__":
    main()
