#!/usr/bin/env python3
"""A/B of the K split inside a skinny-batch bf16 chain launch (xsmm_hip_set_chain_skinny_split) on one GPU, after
tools/chain_skinny_f32_ab.py --chain-split: the rows of profiles/chain_skinny_ab.txt (tools/chain_skinny_ab.py CHAINS and Step: a rank's MLP step
with m = 1 / 8 / 16 / 31 rows, three layers, bias + relu, device-resident operands, asynchronous mode), timed with events around --iters steps.
Per round:
    a       the calls one by one under set_skinny_bf16(1) + set_skinny_split(1) on the PARENT commit's library: THE BASELINE; one child
            process per round for all rows, under its own `timeout`
    u<BN>   the unsplit one launch, set_chain_skinny(BN), for every BN with an instance
    <BN>/P  the K-split one launch, set_chain_skinny(BN) + set_chain_skinny_split(P), P 2 / 4 / 8
and the median [min .. max] of each side in us per step, with the rounds in which it beat (a). Mode 1 of the new switch may take exactly the
(row class, image, BN, P) that beat (a) in EVERY round. Controls: child processes on the parent's library alternate with child processes on
this tree's with every switch as it starts - a plain 4096-row chain, a single call, and every row call by call.
    python tools/chain_skinny_split_ab.py --parent-root DIR --out profiles/chain_skinny_split_ab.txt"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chain_skinny_ab import CHAINS, MS, Single, Step, name  # noqa: E402

PS = [2, 4, 8]
ROWS = [(m, k0, ns, image) for (k0, ns), images in CHAINS for image in images for m in MS]


def bns(image, ns):
    return [bn for bn in (16, 32, 64) if not (image == 0 and bn == 16) and min(ns) >= bn]


def warm(s, iters):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.05:
        s.timed(iters)


def child(root, iters, side_a):
    """on the library of the tree at `root`, one JSON line of us per step: side (a) of every row, or the controls with every switch as it starts"""
    sys.path.insert(0, root)
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    rt.set_async(True)
    rows = [] if side_a else [("4096 rows x 3 layers of 1024, plain chain", lambda: Step(rt, 4096, 1024, [1024] * 3)), ("single call 1024 x 1024 x 1024", lambda: Single(rt))]
    rows += [(("" if side_a else "mode 0: ") + name(m, k0, ns, image), lambda m=m, k0=k0, ns=ns, image=image: Step(rt, m, k0, ns, image)) for m, k0, ns, image in ROWS]
    if side_a:
        rt.set_skinny_bf16(1), rt.set_skinny_split(1)
    out = {}
    for what, make in rows:
        s = make()
        warm(s, iters)
        out[what] = s.timed(iters)[0]
    print(json.dumps(out))


def run_child(args, what, root):
    """a child process of this tool under its own time limit; a child that failed or ran into its limit ends the tool: nothing more is
    started on the GPU"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_") and k != "TPP_XSMM_LIBRARY"}
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), what, root, "--iters", str(args.iters)], capture_output=True, text=True, env=env)
    if p.returncode != 0:
        print("# child %s on %s ended with %d: %s" % (what, root, p.returncode, p.stderr[-400:].replace("\n", " ")), flush=True)
        sys.exit(p.returncode)
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--child-side-a", default="", help="(internal) time side (a) on the tree at this root and print JSON")
    ap.add_argument("--child-control", default="", help="(internal) run the controls on the tree at this root and print JSON")
    args = ap.parse_args()
    if args.child_side_a or args.child_control:
        return child(args.child_side_a or args.child_control, args.iters, bool(args.child_side_a))
    if not args.parent_root:
        ap.error("--parent-root: side (a) and the controls run on the parent commit's library")
    parent = os.path.abspath(args.parent_root)
    sys.path.insert(0, ROOT)
    import torch
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    torch.cuda.set_device(0)
    rt.set_async(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def set_side(side):
        rt.set_chain_skinny(side[0] if side else 0), rt.set_chain_skinny_split(side[1] if side else 0)
    props = torch.cuda.get_device_properties(0)
    say("# the K split inside a skinny-batch bf16 chain launch (xsmm_hip_set_chain_skinny_split): the parent's split calls against one launch; one GPU")
    say("# box: %s, %d CUs; bias + relu; command: tools/chain_skinny_split_ab.py --parent-root <parent checkout> --iters %d --rounds %d" % (props.name, props.multi_processor_count, args.iters, args.rounds))
    say("# %d steps between two events, %d alternating rounds; us per step: median [min .. max]; a = calls under skinny_bf16(1) + skinny_split(1) on the PARENT's library (a child "
        "process per round); uBN = set_chain_skinny(BN) unsplit; BN/P = + set_chain_skinny_split(P); (P, G) of the launch; wins = rounds faster than a" % (args.iters, args.rounds))
    rows = [(m, k0, ns, image, Step(rt, m, k0, ns, image)) for m, k0, ns, image in ROWS]
    sides = lambda image, ns: [(bn, P) for bn in bns(image, ns) for P in [0] + PS]  # noqa: E731
    label = lambda side: "u%d" % side[0] if side[1] == 0 else "%d/%d" % side  # noqa: E731
    for m, k0, ns, image, s in rows:  # clocks up, every side warm
        for side in sides(image, ns):
            set_side(side)
            s.timed(args.iters)
    us, how = {}, {}
    for rnd in range(args.rounds):
        print("round %d of %d" % (rnd + 1, args.rounds), file=sys.stderr, flush=True)
        set_side(None)
        for what, t in run_child(args, "--child-side-a", parent).items():
            us.setdefault((what, "a"), []).append(t)
        for m, k0, ns, image, s in rows:
            for side in sides(image, ns):
                set_side(side)
                before, sbefore = rt.chain_skinny_stats()[0], rt.chain_skinny_split_stats()[0]
                t, fused = s.timed(args.iters)
                st, sst = rt.chain_skinny_stats(), rt.chain_skinny_split_stats()
                ok = fused and st[0] > before and (sst[0] > sbefore) == (side[1] != 0)
                how[(name(m, k0, ns, image), side)] = ("G %d" % st[1] if side[1] == 0 else "P %d G %d" % sst[1:3]) if ok else "NOT THIS FORM"
                us.setdefault((name(m, k0, ns, image), side), []).append(t)
    set_side(None)
    for m, k0, ns, image, s in rows:
        what = name(m, k0, ns, image)
        a = us[(what, "a")]
        say(what)
        say("    %-5s %8.2f [%8.2f .. %8.2f]  %-14s    rounds: %s" % ("a", statistics.median(a), min(a), max(a), "calls, parent", " ".join("%.2f" % v for v in a)))
        for side in sides(image, ns):
            v = us[(what, side)]
            say("    %-5s %8.2f [%8.2f .. %8.2f]  %-14s %+6.1f %% against a, wins %d / %d   rounds: %s" % (
                label(side), statistics.median(v), min(v), max(v), how[(what, side)], 100.0 * (statistics.median(v) - statistics.median(a)) / statistics.median(a),
                sum(y < x for x, y in zip(a, v)), args.rounds, " ".join("%.2f" % y for y in v)))
    say("# what set_chain_skinny(1) + set_chain_skinny_split(1) does with each row (gemm_plan.cpp plan_chain_skinny)")
    for m, k0, ns, image, s in rows:
        set_side((1, 1))
        before, sbefore = rt.chain_skinny_stats()[0], rt.chain_skinny_split_stats()[0]
        s.run()
        rt.synchronize()
        st, sst = rt.chain_skinny_stats(), rt.chain_skinny_split_stats()
        say("    %-48s %s" % (name(m, k0, ns, image), "calls" if not (s.fused and st[0] > before) else "G %d BN %d" % st[1:3] + (" P %d" % sst[1] if sst[0] > sbefore else " unsplit")))
    set_side(None)
    say("# controls against the parent commit's library: child processes - the parent's, this tree's with every switch as it starts - alternating (and alternating in who goes first), %d each" % args.rounds)
    order = [("this tree", ROOT), ("parent", parent)]
    got = {who: {} for who, _ in order}
    for pair in range(args.rounds):
        for who, root in (order if pair % 2 == 0 else order[::-1]):  # (the first child of a round finds the clocks lower)
            for what, t_us in run_child(args, "--child-control", root).items():
                got[who].setdefault(what, []).append(t_us)
    for what, a in got["parent"].items():
        b = got["this tree"][what]
        say("%-60s parent %8.2f [%8.2f .. %8.2f] | this tree %8.2f [%8.2f .. %8.2f] %+5.1f %% %s" % (
            what, statistics.median(a), min(a), max(a), statistics.median(b), min(b), max(b), 100.0 * (statistics.median(b) - statistics.median(a)) / statistics.median(a),
            "inside the parent's spread" if min(a) <= statistics.median(b) <= max(a) else "OUTSIDE the parent's spread"))
    say("# not measured: other CU counts, several ranks, layers between the measured sizes, P 3 and P beyond 8, small flat and VNNI-4 chains")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
