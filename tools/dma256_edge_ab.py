#!/usr/bin/env python3
"""A/B of the edge tiles of the 256x256 bf16 tile (xsmm_hip_set_dma256_edge) on one GPU: whole-layer bf16 calls (k = 64
wide batch elements, br = K / 64, beta 0 + bias + relu) on device-resident operands in asynchronous mode, timed with events around --iters
invokes. Every row is warmed up on all its sides, then runs --pairs alternating rounds of three sides:
    off   every switch off (what the library does by default)
    et2   xsmm_hip_set_edge_tiles(2), the loader-wave edge tiles: the best a caller could ask for before this switch
    on    xsmm_hip_set_dma256_edge(2)
and reports median, min and max of each side, in how many rounds `on` was faster than each of the other two, and whether mode 1 (the rule)
takes the row. A row GAINS only if `on` is faster in the majority of the rounds against BOTH other sides.
--controls: divisible shapes, switch off / switch on (the switch must not touch them). With --root <a checkout of another commit, built> the
same rows run on that library (sides it has no setter for are left out): run the two alternately for a parent / tree comparison.
    python tools/dma256_edge_ab.py --out profiles/dma256_edge_ab.txt"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, VB = 2, 2048

# image (0 flat, 2 VNNI-2, 4 VNNI-4), m, n, K
ROWS = [(2, 4000, 4096, 1024), (2, 4096, 4000, 1024), (2, 4100, 4096, 1024), (2, 5000, 5000, 1024), (2, 8000, 8000, 1024), (2, 16000, 1024, 1024),
        (0, 4000, 4096, 1024), (4, 4000, 4096, 1024), (0, 8000, 8000, 1024), (4, 8000, 8000, 1024)]
CONTROLS = [(2, 4096, 4096, 1024), (2, 16384, 1024, 1024)]
INAME = {0: "flat", 2: "VNNI-2", 4: "VNNI-4"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--controls", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    has_switch = hasattr(rt, "set_dma256_edge")
    torch.cuda.set_device(0)
    rt.set_async(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    try:
        commit = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    say("# edge tiles on the 256x256 bf16 tile (xsmm_hip_set_dma256_edge): %s, one process, one GPU" % ("controls" if args.controls else "off / et2 / on"))
    say("# box: %s, %d CUs; commit of the library's tree: %s, %s the switch; command: %s" % (
        props.name, props.multi_processor_count, commit, "with" if has_switch else "WITHOUT", " ".join(sys.argv)))
    say("# per side: %d invokes between two events, %d alternating rounds; us per invoke: median [min .. max]" % (args.iters, args.pairs))
    for image, m, n, K in (CONTROLS if args.controls else ROWS):
        k, br = 64, K // 64
        A = (torch.rand(m, K, device="cuda") * 2 - 1).to(torch.bfloat16)
        B = (torch.rand(K * n, device="cuda") - 0.5).to(torch.bfloat16)  # uniform data: the same buffer serves every image
        C = torch.zeros(m, n, device="cuda", dtype=torch.bfloat16)
        D = (torch.rand(n, device="cuda") * 2 - 1).to(torch.bfloat16)
        old = rt.set_vnni_factor(image) if image else None
        h = rt.fused_brgemm_dispatch(BF16, m, n, k, K, n, n, k, k * n, 4 | (VB if image else 0), 0, 5, 4, 1)
        if image:
            rt.set_vnni_factor(old)

        def run():
            rt.fused_brgemm(BF16, h, A, 0, B, 0, C, 0, D, 0, br)

        def side(which):
            if which == "et2":
                rt.set_edge_tiles(2)
            if which == "on":
                rt.set_dma256_edge(2)
            run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            rt.set_edge_tiles(0)
            if has_switch:
                rt.set_dma256_edge(0)
            return e0.elapsed_time(e1) * 1e3 / args.iters, rt.last_refined_kernel() or rt.kernel_name(h)

        sides = ["off"] + ([] if args.controls else ["et2"]) + (["on"] if has_switch else [])
        rule = "-"
        if has_switch:
            rt.set_dma256_edge(1)
            before = rt.dma256_edge_stats()[0]
            run()
            torch.cuda.synchronize()
            rule = "takes it" if rt.dma256_edge_stats()[0] > before else "refuses"
            rt.set_dma256_edge(0)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:  # clocks up, every kernel warm
            for s in sides:
                side(s)
        t, names = {s: [] for s in sides}, {}
        for _ in range(args.pairs):
            for s in sides:
                us, names[s] = side(s)
                t[s].append(us)
        med = {s: statistics.median(t[s]) for s in sides}
        say("%-6s %5d x %5d x %4d  tiles %3d x %3d  mode 1 %s" % (INAME[image], m, n, K, -(-m // 256), -(-n // 256), rule))
        for s in sides:
            say("    %-3s %8.2f [%8.2f .. %8.2f]  %7.1f TF  %s" % (s, med[s], min(t[s]), max(t[s]), 2.0 * m * n * K / med[s] * 1e-6, names[s]))
        if "on" in sides:
            wins = {s: sum(b < a for a, b in zip(t[s], t["on"])) for s in sides if s != "on"}
            gains = all(2 * w > args.pairs for w in wins.values())
            say("    on against " + ", ".join("%s %+6.1f %% (faster in %d of %d rounds)" % (s, 100.0 * (med["on"] - med[s]) / med[s], wins[s], args.pairs) for s in wins) +
                (": unchanged expected" if args.controls else ": GAINS" if gains else ": does not gain"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
