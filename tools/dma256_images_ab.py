#!/usr/bin/env python3
"""A/B of the flat and VNNI-4 B images of the 256x256 bf16 tile (xsmm_hip_set_dma256_images) on one GPU: whole-layer bf16
calls (k = 64 chunks, br = K / 64, beta 0) on device-resident operands in asynchronous mode, timed with events around --iters invokes.
Every row is warmed up in both modes, then runs --pairs alternating pairs switch off / switch on - mode 1, or mode 2 where the rule
refuses the shape (marked) - and reports median, min and max of each side. The VNNI-2 rows of the same shapes run in the same session as the
yardstick: both of their sides are the kernel the new images extend.
A row counts as FASTER only if every pair is faster and the median gain exceeds the spread (max - min) of the row's switch-off runs;
SLOWER the same way round; else "no difference shown".
    python tools/dma256_images_ab.py --out profiles/dma256_images_ab.txt"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF16, VB = 2, 2048

# m, n, K, bias + relu, what
ROWS = [
    (4096, 4096, 4096, False, "4096^3"),
    (8192, 8192, 1024, False, "8192x8192x1024"),
    (4096, 4096, 1024, False, "4096x4096x1024"),
    (16384, 1024, 1024, True, "16384x1024x1024 bias relu (a layer of the chain-rounds gate)"),
    (32768, 1024, 1024, True, "32768x1024x1024 bias relu (a layer of the chain-rounds gate)"),
    (3840, 4096, 1024, False, "3840x4096x1024 (240 tiles: the rule's edge)"),
    (2048, 2048, 2048, False, "2048^3 (64 tiles, mode 2: the control, expected slower)"),
]
IMAGES = [(0, "flat"), (4, "VNNI-4"), (2, "VNNI-2")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    torch.cuda.set_device(0)
    rt.set_async(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    say("# flat and VNNI-4 B on the 256x256 bf16 tile (xsmm_hip_set_dma256_images): switch off against switch on, one process, one GPU")
    say("# box: %s, %d CUs; parent commit of this tree: %s; command: %s" % (props.name, props.multi_processor_count, commit, " ".join(sys.argv)))
    say("# per side: %d invokes between two events, %d alternating pairs; us per invoke: median [min .. max]" % (args.iters, args.pairs))
    for m, n, K, fused, what in ROWS:
        if args.only and args.only not in what:
            continue
        k, br = 64, K // 64
        A = (torch.rand(m, K, device="cuda") * 2 - 1).to(torch.bfloat16)
        B = (torch.rand(K * n, device="cuda") - 0.5).to(torch.bfloat16)  # uniform data: the same buffer serves every image
        C = torch.zeros(m, n, device="cuda", dtype=torch.bfloat16)
        D = (torch.rand(n, device="cuda") * 2 - 1).to(torch.bfloat16)
        for image, iname in IMAGES:
            old = rt.set_vnni_factor(image) if image else None
            flags = 4 | (VB if image else 0)
            if fused:
                h = rt.fused_brgemm_dispatch(BF16, m, n, k, K, n, n, k, k * n, flags, 0, 5, 4, 1)
            else:
                h = rt.brgemm_dispatch(BF16, m, n, k, K, n, n, k, k * n, flags)
            if image:
                rt.set_vnni_factor(old)

            def run():
                if fused:
                    rt.fused_brgemm(BF16, h, A, 0, B, 0, C, 0, D, 0, br)
                else:
                    rt.brgemm(BF16, h, A, 0, B, 0, C, 0, br)

            def side(mode):
                rt.set_dma256_images(mode)
                run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    run()
                e1.record()
                torch.cuda.synchronize()
                rt.set_dma256_images(0)
                return e0.elapsed_time(e1) * 1e3 / args.iters, rt.last_refined_kernel() or rt.kernel_name(h)

            # the mode the row runs under: 1, or 2 where the rule refuses
            rt.set_dma256_images(1)
            before = rt.dma256_images_stats()[0]
            run()
            torch.cuda.synchronize()
            on = 1 if rt.dma256_images_stats()[0] > before or image == 2 else 2
            rt.set_dma256_images(0)
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.2:  # clocks up, both kernels warm
                side(0), side(on)
            offs, ons, names = [], [], {}
            for _ in range(args.pairs):
                a, names[0] = side(0)
                b, names[1] = side(on)
                offs.append(a), ons.append(b)
            med0, med1 = statistics.median(offs), statistics.median(ons)
            spread = max(offs) - min(offs)
            if all(b < a for a, b in zip(offs, ons)) and med0 - med1 > spread:
                verdict = "FASTER"
            elif all(b > a for a, b in zip(offs, ons)) and med1 - med0 > spread:
                verdict = "SLOWER"
            else:
                verdict = "no difference shown"
            fl = 2.0 * m * n * K
            say("%-8s %-62s off %8.2f [%8.2f .. %8.2f] %-32s | mode %d %8.2f [%8.2f .. %8.2f] %-32s | %+6.1f %% %7.1f -> %7.1f TF  %s" % (
                iname, what, med0, min(offs), max(offs), names[0], on, med1, min(ons), max(ons), names[1], 100.0 * (med1 - med0) / med0,
                fl / med0 * 1e-6, fl / med1 * 1e-6, verdict if image != 2 else "(yardstick: the same kernel on both sides)"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
