#!/usr/bin/env python3
"""A/B of the narrow-output bf16 kernel (xsmm_hip_set_narrow_bf16) against mode 0 - the parent commit's kernels, unchanged -
on one GPU, in ONE process. Whole-layer bf16 calls with m >= 32 rows and n <= 31 columns (beta 0 + bias + relu, packed operands) on
device-resident operands in asynchronous mode, timed with events around --iters invokes after a warm-up of both sides.
    python tools/narrow_bf16_ab.py --out profiles/narrow_bf16_ab.txt
Per row and forced BM (16, 32, 64): --rounds ALTERNATING pairs (mode 0, the BM). A BM counts as faster only if it beat mode 0 in EVERY
pair; mode 1 (gemm_plan.cpp narrow_bf16_bm) may take a BM only there. The spread of each side is its [min .. max] over the pairs. The last
column of a row is what mode 1 does with it."""
import argparse
import importlib
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, VB = 2, 2048
# m, n, k per batch element, batch elements, B image (2 VNNI-2, 0 flat, 4 VNNI-4)
ROWS = [(1024, 10, 128, 1, 2), (4096, 10, 1024, 1, 2), (256, 16, 1024, 1, 2), (65536, 1, 1024, 1, 2), (4096, 31, 4096, 1, 2), (4096, 10, 1000, 1, 2),
        (4096, 16, 1024, 1, 2), (4096, 8, 1024, 1, 2), (65536, 10, 1024, 1, 2), (512, 10, 512, 1, 2), (4096, 10, 64, 16, 2),
        (32, 10, 128, 1, 2), (64, 31, 64, 1, 2), (128, 10, 1024, 1, 2), (4096, 10, 32, 1, 2), (4096, 17, 8, 1, 2), (1024, 31, 128, 1, 2), (32, 16, 4096, 1, 2),
        (4096, 10, 1024, 1, 0), (4096, 31, 4096, 1, 0), (1024, 10, 128, 1, 0), (256, 16, 1024, 1, 0), (32, 10, 128, 1, 0),
        (4096, 10, 1024, 1, 4), (4096, 31, 4096, 1, 4), (1024, 10, 128, 1, 4), (256, 16, 1024, 1, 4), (32, 10, 128, 1, 4)]
IMAGE = {2: "VNNI-2", 0: "flat", 4: "VNNI-4"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    sys.path.insert(0, HERE)
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    torch.cuda.set_device(0)
    rt.set_async(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(run, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    props = torch.cuda.get_device_properties(0)
    say("# narrow-output bf16 layers (xsmm_hip_set_narrow_bf16): mode 0 (the parent commit's kernels) against each forced BM, one process")
    say("# box: %s, %d CUs; command: tools/narrow_bf16_ab.py --iters %d --rounds %d" % (props.name, props.multi_processor_count, args.iters, args.rounds))
    say("# per side: %d invokes between two events after 20 warm-up invokes; %d alternating pairs (mode 0, BM); us per invoke: median [min .. max]" % (args.iters, args.rounds))
    say("# wins: pairs in which the BM beat the mode 0 of the same pair; TB/s: the bytes of A (2 m k br) over the median")
    for m, n, k, br, image in ROWS:
        K = k * br
        A, B = ((torch.rand(s, device="cuda") - 0.5).bfloat16().view(torch.int16) for s in (m * K, K * n))
        D, C = (torch.rand(n, device="cuda") - 0.5).bfloat16().view(torch.int16), torch.zeros(m * n, dtype=torch.int16, device="cuda")
        old = rt.set_vnni_factor(image) if image else None
        h = rt.fused_brgemm_dispatch(BF16, m, n, k, K, n, n, k, k * n, 4 | (VB if image else 0), 0, 5, 4, 1)
        if image:
            rt.set_vnni_factor(old)

        def run():
            rt.fused_brgemm(BF16, h, A, 0, B, 0, C, 0, D, 0, br)

        def side(mode):
            rt.set_narrow_bf16(mode)
            for _ in range(20):
                run()
            t = timed(run, args.iters)
            name = rt.last_refined_kernel() or rt.kernel_name(h)
            rt.set_narrow_bf16(0)
            return t, name

        rt.set_narrow_bf16(1)
        before = rt.narrow_bf16_stats()[0]
        run()
        torch.cuda.synchronize()
        rule = "BM %d" % rt.narrow_bf16_stats()[3] if rt.narrow_bf16_stats()[0] > before else "gates"
        rt.set_narrow_bf16(0)
        say("%d x %d x %d br %d %s  mode 1: %s" % (m, n, k, br, IMAGE[image], rule))
        for bm in (16, 32, 64):
            pairs = [(side(0), side(bm)) for _ in range(args.rounds)]
            off, on = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
            fmt = lambda v: "%8.2f [%8.2f .. %8.2f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
            say("    off   %s  %s" % (fmt(off), pairs[0][0][1]))
            say("    %-5d %s  %+6.1f %%  %5.2f TB/s  wins %d of %d  %s" % (bm, fmt(on), 100 * (statistics.median(on) / statistics.median(off) - 1),
                                                                         2.0 * m * K / statistics.median(on) * 1e-6, sum(b < a for a, b in zip(off, on)), args.rounds, pairs[0][1][1]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
