#!/usr/bin/env python3
"""A/B of the K split across workgroups of the skinny-batch f32 kernel (xsmm_hip_set_skinny_f32_split) on one GPU: the rows
of tools/skinny_f32_ab.py (n x K 1024^2, 1000^2, 4096 x 1024, 1024 x 4096, 4096^2 at m 1 / 8 / 16 / 17 / 31, beta 0 + bias + relu) under
forced BN 16 and 32 (and 64 on 1024 x 4096) x P 2 / 4 / 8 / 16, each timed against the UNSPLIT skinny launch of the same BN in the same
child process, the generic kernel's time alongside.
    python tools/skinny_f32_split_ab.py --parent <a checkout of the parent commit, built> --out profiles/skinny_f32_split_ab.txt
Each of --rounds rounds starts two child processes, one after the other: the parent's library (switches off, and the unsplit skinny launch
of every forced BN) and this tree's (the same, and every P). A P counts as faster in a round only if it beat the unsplit launch of that
round; mode 1 may take a (row class, BN, P) only where that holds in EVERY round. Controls: with both switches off every row and the 1024^3
f32 call (C2), and every unsplit skinny row, against the parent's own [min .. max]."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = 1
SHAPES = [(1024, 1024), (1000, 1000), (4096, 1024), (1024, 4096), (4096, 4096)]  # n x K
MS = (1, 8, 16, 17, 31)
PS = (2, 4, 8, 16)


def bns(n, K):
    return (16, 32, 64) if (n, K) == (1024, 4096) else (16, 32)


def child(root, iters, split):
    import torch
    sys.path.insert(0, root)
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    torch.cuda.set_device(0)
    rt.set_async(True)
    out = {}

    def timed(run):
        for _ in range(20):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def row(name, m, n, K, fused, sides):
        k, br = (64, K // 64) if K % 64 == 0 else (K, 1)
        A, B, D = torch.rand(m, K, device="cuda") * 2 - 1, torch.rand(K, n, device="cuda") - 0.5, torch.rand(n, device="cuda") * 2 - 1
        C = torch.zeros(m, n, device="cuda")
        h = rt.fused_brgemm_dispatch(F32, m, n, k, K, n, n, k, k * n, 4, 0, 5, 4, 1) if fused else rt.brgemm_dispatch(F32, m, n, k, K, n, n, k, k * n, 4)
        run = (lambda: rt.fused_brgemm(F32, h, A, 0, B, 0, C, 0, D, 0, br)) if fused else (lambda: rt.brgemm(F32, h, A, 0, B, 0, C, 0, br))
        out[name + " off"] = [timed(run), rt.last_refined_kernel() or rt.kernel_name(h)]
        for bn in sides:
            rt.set_skinny_f32(bn)
            out["%s %d" % (name, bn)] = [timed(run), rt.last_refined_kernel()]
            for P in PS if split else ():
                rt.set_skinny_f32_split(P)
                out["%s %d/%d" % (name, bn, P)] = [timed(run), rt.last_refined_kernel()]
                rt.set_skinny_f32_split(0)
            rt.set_skinny_f32(0)
        if split and sides:  # what mode 1 of both switches does with the row
            rt.set_skinny_f32(1), rt.set_skinny_f32_split(1)
            before = rt.skinny_f32_stats()[0], rt.skinny_f32_split_stats()[0]
            run()
            torch.cuda.synchronize()
            s, p = rt.skinny_f32_stats(), rt.skinny_f32_split_stats()
            out[name + " rule"] = "gates" if s[0] == before[0] else "BN %d" % s[3] + (" P %d" % p[1] if p[0] > before[1] else " unsplit")
            rt.set_skinny_f32(0), rt.set_skinny_f32_split(0)

    row("C2 1024x1024x1024", 1024, 1024, 1024, False, ())
    for n, K in SHAPES:
        for m in MS:
            row("n %4d K %4d m %2d" % (n, K, m), m, n, K, True, bns(n, K))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--split", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.iters, args.split)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(root, split):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(root), "--iters", str(args.iters), "--split", str(split)],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.exit("a child failed (%d):\n%s" % (p.returncode, p.stderr[-3000:]))
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])

    Pa, T = [], []
    for _ in range(args.rounds):
        Pa.append(run(args.parent, 0)), T.append(run(HERE, 1))
    import torch
    props = torch.cuda.get_device_properties(0)
    say("# K split of the skinny-batch f32 kernel (xsmm_hip_set_skinny_f32_split): parent / tree alternating, a child process each")
    say("# box: %s, %d CUs; command: %s" % (props.name, props.multi_processor_count, " ".join(sys.argv)))
    say("# per side: %d invokes between two events after 20 warm-up invokes, %d rounds; us per invoke: median [min .. max]" % (args.iters, args.rounds))
    say("# BN/P lines: against the unsplit skinny launch of the same BN in the same child; wins: rounds in which the split was faster")
    say("# control lines (off, BN unsplit): this tree against the parent's own [min .. max] over its %d runs" % args.rounds)

    def fmt(v):
        return "%8.2f [%8.2f .. %8.2f]" % (statistics.median(v), min(v), max(v))

    for name in [k[:-4] for k in T[0] if k.endswith(" off")]:
        say("%s  generic: %s%s" % (name, T[0][name + " off"][1], "  mode 1 + 1: " + T[0][name + " rule"] if name + " rule" in T[0] else ""))
        for side in [k[len(name) + 1:] for k in T[0] if k.startswith(name + " ") and not k.endswith(" rule")]:
            t = [r["%s %s" % (name, side)][0] for r in T]
            if "/" not in side:  # a control: the parent has this side too
                p = [r["%s %s" % (name, side)][0] for r in Pa]
                say("    %-6s %s   parent %s  %+5.1f %%: %s the parent's spread" % (side, fmt(t), fmt(p), 100 * (statistics.median(t) / statistics.median(p) - 1),
                                                                                   "within" if min(p) <= statistics.median(t) <= max(p) else "OUTSIDE"))
            else:
                u = [r["%s %s" % (name, side.split("/")[0])][0] for r in T]
                say("    %-6s %s   %+5.1f %%  wins %d of %d" % (side, fmt(t), 100 * (statistics.median(t) / statistics.median(u) - 1), sum(a < b for a, b in zip(t, u)), args.rounds))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
