#!/usr/bin/env python3
"""A/B of the skinny-batch f32 kernel (xsmm_hip_set_skinny_f32) against the PARENT commit's library on one GPU. Whole-layer
f32 calls with m < 32 rows (k = 64 wide batch elements where 64 divides K, else one batch element of K; beta 0 + bias + relu) on
device-resident operands in asynchronous mode, timed with events around --iters invokes after a warm-up of every side.
    python tools/skinny_f32_ab.py --parent <a checkout of the parent commit, built> --out profiles/skinny_f32_ab.txt
Each of --rounds rounds starts four child processes, one after the other: the parent's library (P), this tree's with the switch off
(T0: the same sequence of calls as P), the parent's again (P2), this tree's with every forced BN (16, 32, 64). The ten runs P and P2 are
the parent's own spread [min .. max]. A forced BN counts as faster in a round only if it beat BOTH parent runs of that round; mode 1 may
take a (row class, BN) only where that holds in EVERY round. Controls, switch off (T0): every row and the 1024 x 1024 x 1024 f32 call (C2)
against the parent - the median of each must sit within the parent's spread."""
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


def child(root, iters, forced):
    import torch
    sys.path.insert(0, root)
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    sides = ["off"] + ([16, 32, 64] if forced else [])
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

    def row(name, m, n, K, flags, fused, only_off=False):
        k, br = (64, K // 64) if K % 64 == 0 else (K, 1)
        A, B, D = torch.rand(m, K, device="cuda") * 2 - 1, torch.rand(K, n, device="cuda") - 0.5, torch.rand(n, device="cuda") * 2 - 1
        C = torch.zeros(m, n, device="cuda")
        h = rt.fused_brgemm_dispatch(F32, m, n, k, K, n, n, k, k * n, flags, 0, 5 if fused else 0, 4 if fused else 0, 1 if fused else 0) if fused else \
            rt.brgemm_dispatch(F32, m, n, k, K, n, n, k, k * n, flags)
        run = (lambda: rt.fused_brgemm(F32, h, A, 0, B, 0, C, 0, D, 0, br)) if fused else (lambda: rt.brgemm(F32, h, A, 0, B, 0, C, 0, br))
        for s in sides[:1] if only_off else sides:
            if s != "off":
                rt.set_skinny_f32(s)
            out["%s %s" % (name, s)] = [timed(run), rt.last_refined_kernel() or rt.kernel_name(h)]
            if s != "off":
                rt.set_skinny_f32(0)
        if forced and not only_off:  # what mode 1 does with the row
            rt.set_skinny_f32(1)
            before = rt.skinny_f32_stats()[0]
            run()
            torch.cuda.synchronize()
            out[name + " rule"] = "BN %d" % rt.skinny_f32_stats()[3] if rt.skinny_f32_stats()[0] > before else "gates"
            rt.set_skinny_f32(0)

    row("C2 1024x1024x1024", 1024, 1024, 1024, 4, False, only_off=True)
    for n, K in SHAPES:
        for m in MS:
            row("n %4d K %4d m %2d" % (n, K, m), m, n, K, 4, True)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--forced", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.iters, args.forced)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(root, forced=0):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(root), "--iters", str(args.iters), "--forced", str(forced)],
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("a child failed (%d):\n%s" % (p.returncode, p.stderr[-3000:]))
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])

    P, T0, P2, T = [], [], [], []
    for _ in range(args.rounds):
        P.append(run(args.parent)), T0.append(run(HERE)), P2.append(run(args.parent)), T.append(run(HERE, 1))
    import torch
    props = torch.cuda.get_device_properties(0)
    say("# skinny-batch f32 layers (xsmm_hip_set_skinny_f32) against the parent commit's library: P / T0 (tree, switch off) / P2 / tree (16, 32, 64), a child process each")
    say("# box: %s, %d CUs; command: %s" % (props.name, props.multi_processor_count, " ".join(sys.argv)))
    say("# per side: %d invokes between two events after 20 warm-up invokes, %d rounds; us per invoke: median [min .. max]; B bytes / median" % (args.iters, args.rounds))
    say("# wins: rounds in which the side beat BOTH parent runs of the round; the parent's spread: [min .. max] of its ten runs")

    def fmt(v):
        return "%8.2f [%8.2f .. %8.2f]" % (statistics.median(v), min(v), max(v))

    for name in [k[:-4] for k in T[0] if k.endswith(" off")]:
        p, p2 = [r[name + " off"][0] for r in P], [r[name + " off"][0] for r in P2]
        nbytes = 4.0 * int(name.split()[1]) * int(name.split()[3]) if name.startswith("n ") else 0
        say("%s  parent: %s%s" % (name, P[0][name + " off"][1], "  mode 1: " + T[0][name + " rule"] if name + " rule" in T[0] else ""))
        say("    P     %s\n    P2    %s" % (fmt(p), fmt(p2)))
        med_p = statistics.median(p + p2)
        t0 = [r[name + " off"][0] for r in T0]
        say("    off   %s   %+5.1f %% against the parent's median: %s the parent's spread [%.2f .. %.2f]" % (
            fmt(t0), 100 * (statistics.median(t0) - med_p) / med_p, "within" if min(p + p2) <= statistics.median(t0) <= max(p + p2) else "OUTSIDE", min(p + p2), max(p + p2)))
        for s in ("16", "32", "64"):
            if name + " " + s in T[0]:
                t = [r[name + " " + s][0] for r in T]
                rel = (statistics.median(t) - med_p) / med_p
                wins = sum(x < min(a, b) for x, a, b in zip(t, p, p2))
                say("    %-5s %s   %+5.1f %%  %5.2f TB/s  wins %d of %d  %s" % (s, fmt(t), 100 * rel, nbytes / statistics.median(t) * 1e-6, wins, args.rounds, T[0][name + " " + s][1]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
