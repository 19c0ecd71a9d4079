#!/usr/bin/env python3
"""A/B of the narrow-output f32 kernel (xsmm_hip_set_narrow_f32) against mode 0 - the parent commit's kernels, unchanged -
on one GPU, in ONE process. Whole-layer f32 calls with m >= 32 rows and n <= 31 columns (beta 0 + bias + relu, packed operands) on
device-resident operands in asynchronous mode, timed with events around --iters invokes after a warm-up of both sides.
    python tools/narrow_f32_ab.py --out profiles/narrow_f32_ab.txt
    python tools/narrow_f32_ab.py --rule-only --out profiles/narrow_f32_ab.txt      (appends what mode 1 does with each row, after fitting)
Per row and forced BM (16, 32, 64): --rounds ALTERNATING pairs (mode 0, the BM). A BM counts as faster only if it beat mode 0 in EVERY
pair; mode 1 (gemm_plan.cpp narrow_f32_bm) may take a BM only there. The spread of each side is its [min .. max] over the pairs. CONTROL
rows are calls dispatch puts on brgemm_f32_lw16<32x16>: no mode takes them, both sides of a pair run the same kernel and must not move."""
import argparse
import importlib
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = 1
# m, n, k per batch element, batch elements
ROWS = [(1024, 10, 128, 1), (4096, 10, 1024, 1), (65536, 1, 1024, 1), (65536, 10, 1024, 1), (4096, 31, 4096, 1), (4096, 10, 1000, 1), (4096, 10, 64, 16),
        (16384, 16, 1024, 1), (65536, 16, 256, 1), (4096, 1, 1024, 1), (4096, 2, 256, 1), (512, 10, 512, 1), (128, 10, 1024, 1), (32, 10, 128, 1), (40, 10, 36, 1),
        (64, 31, 64, 1), (1024, 31, 128, 1), (4096, 10, 16, 1), (4096, 17, 16, 1), (16384, 31, 512, 1), (32, 31, 4096, 1),
        # n % 4 == 0, where the generic kernel reads B and writes C in 16-byte pieces, and m between 4096 and 65536
        (8224, 16, 1024, 1), (4096, 8, 1024, 1), (4096, 12, 1024, 1), (16384, 8, 1024, 1), (65536, 4, 1024, 1), (1024, 20, 128, 1), (4096, 28, 4096, 1),
        (40, 12, 36, 1), (8200, 10, 1024, 1), (32768, 10, 1024, 1), (16384, 10, 256, 1),
        (256, 16, 1024, 1), (4096, 16, 1024, 1), (32, 16, 4096, 1)]  # (the last three: controls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rule-only", action="store_true")
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
    if args.rule_only:
        say("# what mode 1 (gemm_plan.cpp narrow_f32_bm, as committed) does with each row; command: tools/narrow_f32_ab.py --rule-only")
    else:
        say("# narrow-output f32 layers (xsmm_hip_set_narrow_f32): mode 0 (the parent commit's kernels) against each forced BM, one process")
        say("# box: %s, %d CUs; command: tools/narrow_f32_ab.py --iters %d --rounds %d" % (props.name, props.multi_processor_count, args.iters, args.rounds))
        say("# per side: %d invokes between two events after 20 warm-up invokes; %d alternating pairs (mode 0, BM); us per invoke: median [min .. max]" % (args.iters, args.rounds))
        say("# wins: pairs in which the BM beat the mode 0 of the same pair; TB/s: the bytes of A (4 m k br) over the median")
    for m, n, k, br in ROWS:
        K = k * br
        A, B, D = (torch.rand(s, device="cuda") - 0.5 for s in (m * K, K * n, n))
        C = torch.zeros(m * n, device="cuda")
        h = rt.fused_brgemm_dispatch(F32, m, n, k, K, n, n, k, k * n, 4, 0, 5, 4, 1)

        def run():
            rt.fused_brgemm(F32, h, A, 0, B, 0, C, 0, D, 0, br)

        def side(mode):
            rt.set_narrow_f32(mode)
            before = rt.narrow_f32_stats()[0]
            for _ in range(20):
                run()
            t = timed(run, args.iters)
            name = rt.last_refined_kernel() or rt.kernel_name(h)
            taken = rt.narrow_f32_stats()[0] > before
            rt.set_narrow_f32(0)
            return t, name, taken

        rt.set_narrow_f32(1)
        before = rt.narrow_f32_stats()[0]
        run()
        torch.cuda.synchronize()
        rule = "BM %d" % rt.narrow_f32_stats()[3] if rt.narrow_f32_stats()[0] > before else "stays on " + (rt.last_refined_kernel() or rt.kernel_name(h))
        rt.set_narrow_f32(0)
        say("%d x %d x %d br %d  mode 1: %s" % (m, n, k, br, rule))
        if args.rule_only:
            continue
        for bm in (16, 32, 64):
            pairs = [(side(0), side(bm)) for _ in range(args.rounds)]
            off, on = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
            fmt = lambda v: "%8.2f [%8.2f .. %8.2f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
            say("    off   %s  %s" % (fmt(off), pairs[0][0][1]))
            say("    %-5d %s  %+6.1f %%  %5.2f TB/s  wins %d of %d  %s%s" % (bm, fmt(on), 100 * (statistics.median(on) / statistics.median(off) - 1),
                                                                           4.0 * m * K / statistics.median(on) * 1e-6, sum(b < a for a, b in zip(off, on)), args.rounds, pairs[0][1][1],
                                                                           "" if pairs[0][1][2] else "  CONTROL: not taken, the same kernel on both sides"))
    if args.out:
        with open(args.out, "a" if args.rule_only else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
