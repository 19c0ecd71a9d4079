#!/usr/bin/env python3
"""A/B of skinny-batch f32 layer chains (xsmm_hip_set_chain_skinny_f32) on one GPU: a rank's MLP step with 1 .. 31 rows - f32,
three layers, bias + relu, device-resident operands, asynchronous mode, whole-layer calls as tpp-mlir_amd/mlp.py dispatches them (64-k batch
elements where 64 divides k) - through xsmm_hip_fused_brgemm_chain_invoke, timed with events around --iters steps. Every row is warmed up on
every side, then runs --rounds alternating rounds of
    a     call by call under set_skinny_f32(1) and set_skinny_f32_split(1): the best existing form, THE BASELINE
    b     call by call with every switch off (the generic kernel)
    16 / 32 / 64   one launch under set_chain_skinny_f32(BN), where every layer is wide enough
and reports the median [min .. max] of each side in us per step and, per one-launch side, in how many rounds it beat (a). Mode 1 may take
exactly the (row, BN) that beat (a) in EVERY round; what set_chain_skinny_f32(1) does with each row is printed behind the rows (--rule-only:
nothing else, no timing).
Controls, with --parent-root DIR (a checkout of the parent commit with its library built): child processes on the parent's library
alternate with child processes on this tree's with every new switch off, each under its own `timeout` - the 4096-row plain bf16 chain of
three 1024-wide layers, the f32 call 1024 x 1024 x 1024, and every row call by call with every switch off (mode 0).
    python tools/chain_skinny_f32_ab.py --out profiles/chain_skinny_f32_ab.txt [--parent-root DIR]
--chain-split (xsmm_hip_set_chain_skinny_f32_split; needs --parent-root): the same rows, three sides per round -
    a       the calls under both single-call switches at 1 on the PARENT commit's library, one child process per round for all rows
    u<BN>   the unsplit one launch on the BN that profiles/chain_skinny_f32_ab.txt found best for the row (32 for 4096-wide, else 16)
    <BN>/P  the K-split one launch under set_chain_skinny_f32(BN) + set_chain_skinny_f32_split(P), BN 16 / 32, P 2 / 4
- and the same controls. Mode 1 of the new switch may take exactly the (row class, BN, P) that beat (a) in EVERY round.
    python tools/chain_skinny_f32_ab.py --chain-split --parent-root DIR --out profiles/chain_skinny_f32_split_ab.txt"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 1, 2
MS = [1, 8, 16, 31]
CHAINS = [(1024, [1024] * 3), (1000, [1000] * 3), (784, [512, 256, 128]), (4096, [4096] * 3)]  # (the input's width, every layer's n)
SIDES = ["a", "b", 16, 32, 64]


def name(m, k0, ns):
    return "m %2d  %d -> %s" % (m, k0, " -> ".join(str(n) for n in ns))


class Step:
    """whole-layer calls of m rows: layer l is [m x k_l] @ [k_l x ns[l]], k_l in 64-k batch elements where 64 divides it; bf16: VNNI-2 weights"""

    def __init__(self, rt, m, k0, ns, dtype=F32):
        import torch
        self.rt, self.torch, self.fused, self.dtype = rt, torch, False, dtype
        t = torch.float32 if dtype == F32 else torch.bfloat16
        ks = [k0] + list(ns[:-1])
        self.brs = [k // 64 if k % 64 == 0 else 1 for k in ks]
        flags = 4 | (2048 if dtype == BF16 else 0)
        self.handles = [rt.fused_brgemm_dispatch(dtype, m, n, k // br, k, n, n, k // br, (k // br) * n, flags, 0, 5, 4, 1) for n, k, br in zip(ns, ks, self.brs)]
        g = torch.Generator().manual_seed(7)
        self.x = (torch.randn(m, k0, generator=g) * 0.5).to(t).cuda()
        self.w = [(torch.randn(k, n, generator=g) * 0.05).to(t).cuda() for n, k in zip(ns, ks)]
        self.b = [(torch.randn(n, generator=g) * 0.1).to(t).cuda() for n in ns]
        self.acts = [torch.zeros(m, n, dtype=t, device="cuda") for n in ns]
        self.run()
        rt.synchronize()

    def run(self):
        cur, calls = self.x, []
        for l, h in enumerate(self.handles):
            calls.append((h, cur, 0, self.w[l], 0, self.acts[l], 0, self.b[l], 0, self.brs[l]))
            cur = self.acts[l]
        self.fused = bool(self.rt.fused_brgemm_chain(self.dtype, calls))

    def timed(self, iters):
        torch = self.torch
        self.run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            self.run()
        e1.record()
        self.rt.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters, self.fused


class Single:
    """the single f32 call 1024 x 1024 x 1024 (bias + relu)"""

    def __init__(self, rt):
        import torch
        self.rt, self.torch, self.fused = rt, torch, False
        self.h = rt.fused_brgemm_dispatch(F32, 1024, 1024, 64, 1024, 1024, 1024, 64, 64 * 1024, 4, 0, 5, 4, 1)
        g = torch.Generator().manual_seed(7)
        self.x, self.w, self.b = (torch.randn(1024, 1024, generator=g) * 0.5).cuda(), (torch.randn(1024, 1024, generator=g) * 0.05).cuda(), (torch.randn(1024, generator=g) * 0.1).cuda()
        self.c = torch.zeros(1024, 1024, device="cuda")

    def run(self):
        self.rt.fused_brgemm(F32, self.h, self.x, 0, self.w, 0, self.c, 0, self.b, 0, 16)

    timed = Step.timed


def set_side(rt, side):
    rt.set_skinny_f32(1 if side == "a" else 0)
    rt.set_skinny_f32_split(1 if side == "a" else 0)
    rt.set_chain_skinny_f32(1 if side == "rule" else side if isinstance(side, int) else 0)


def child_side_a(root, iters):
    """side (a) of --chain-split on the library of the tree at `root`: every row call by call under both single-call f32 skinny switches at 1"""
    sys.path.insert(0, root)
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    rt.set_async(True)
    set_side(rt, "a")
    out = {}
    for k0, ns in CHAINS:
        for m in MS:
            s = Step(rt, m, k0, ns)
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.05:
                s.timed(iters)
            out[name(m, k0, ns)] = s.timed(iters)[0]
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


def chain_split_ab(args, rt, say):
    """--chain-split: per round one child on the parent's library for side (a) of every row, then every row's one-launch sides in this process"""
    parent = os.path.abspath(args.parent_root)
    rows = [(m, k0, ns, Step(rt, m, k0, ns)) for k0, ns in CHAINS for m in MS]
    sides = lambda ns: [("u", 32 if min(ns) >= 4096 else 16, 0)] + [("s", bn, P) for bn in (16, 32) for P in (2, 4)]
    label = lambda side: "u%d" % side[1] if side[0] == "u" else "%d/%d" % side[1:]

    def set_split_side(side):
        rt.set_skinny_f32(0), rt.set_skinny_f32_split(0)
        rt.set_chain_skinny_f32(side[1] if side else 0), rt.set_chain_skinny_f32_split(side[2] if side else 0)
    for m, k0, ns, s in rows:  # clocks up, every side warm
        for side in sides(ns):
            set_split_side(side)
            s.timed(args.iters)
    us, how = {}, {}
    for _ in range(args.rounds):
        set_split_side(None)
        for what, t in run_child(args, "--child-side-a", parent).items():
            us.setdefault((what, "a"), []).append(t)
        for m, k0, ns, s in rows:
            for side in sides(ns):
                set_split_side(side)
                before, sbefore = rt.chain_skinny_f32_stats()[0], rt.chain_skinny_f32_split_stats()[0]
                t, fused = s.timed(args.iters)
                st, sst = rt.chain_skinny_f32_stats(), rt.chain_skinny_f32_split_stats()
                ok = fused and st[0] > before and (sst[0] > sbefore) == (side[0] == "s")
                how[(name(m, k0, ns), side)] = "G %d BN %d W %d" % st[1:4] if ok else "NOT THIS FORM"
                us.setdefault((name(m, k0, ns), side), []).append(t)
    set_split_side(None)
    for m, k0, ns, s in rows:
        what = name(m, k0, ns)
        a = us[(what, "a")]
        say(what)
        say("    %-5s %8.2f [%8.2f .. %8.2f]  %-16s    rounds: %s" % ("a", statistics.median(a), min(a), max(a), "calls, parent", " ".join("%.2f" % v for v in a)))
        for side in sides(ns):
            v = us[(what, side)]
            say("    %-5s %8.2f [%8.2f .. %8.2f]  %-16s %+6.1f %% against a, wins %d / %d   rounds: %s" % (
                label(side), statistics.median(v), min(v), max(v), how[(what, side)], 100.0 * (statistics.median(v) - statistics.median(a)) / statistics.median(a),
                sum(y < x for x, y in zip(a, v)), args.rounds, " ".join("%.2f" % y for y in v)))
    say("# what set_chain_skinny_f32(1) + set_chain_skinny_f32_split(1) does with each row (gemm_plan.cpp plan_chain_skinny_f32)")
    for m, k0, ns, s in rows:
        rt.set_chain_skinny_f32(1), rt.set_chain_skinny_f32_split(1)
        before, sbefore = rt.chain_skinny_f32_stats()[0], rt.chain_skinny_f32_split_stats()[0]
        s.run()
        rt.synchronize()
        st, sst = rt.chain_skinny_f32_stats(), rt.chain_skinny_f32_split_stats()
        say("    %-40s %s" % (name(m, k0, ns), "calls" if not (s.fused and st[0] > before) else "G %d BN %d waves %d" % st[1:4] + (" P %d" % sst[1] if sst[0] > sbefore else " unsplit")))
    set_split_side(None)


def child_control(root, iters):
    """the controls on the library of the tree at `root`, every switch as the library starts; one JSON line of us per step"""
    sys.path.insert(0, root)
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    rt.set_async(True)
    out = {}
    rows = [("4096 rows x 3 layers of 1024, plain bf16 chain", lambda: Step(rt, 4096, 1024, [1024] * 3, BF16)), ("f32 call 1024 x 1024 x 1024", lambda: Single(rt))]
    rows += [("mode 0: " + name(m, k0, ns), lambda m=m, k0=k0, ns=ns: Step(rt, m, k0, ns)) for k0, ns in CHAINS for m in MS]
    for what, make in rows:
        s = make()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:
            s.timed(iters)
        out[what] = s.timed(iters)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--rule-only", action="store_true")
    ap.add_argument("--chain-split", action="store_true", help="the K split inside the launch (xsmm_hip_set_chain_skinny_f32_split) against the parent's calls")
    ap.add_argument("--child-control", default="", help="(internal) run the controls on the tree at this root and print JSON")
    ap.add_argument("--child-side-a", default="", help="(internal) time side (a) of --chain-split on the tree at this root and print JSON")
    args = ap.parse_args()
    if args.child_control:
        return child_control(args.child_control, args.iters)
    if args.child_side_a:
        return child_side_a(args.child_side_a, args.iters)
    if args.chain_split and not args.parent_root:
        ap.error("--chain-split needs --parent-root: side (a) runs on the parent commit's library")
    sys.path.insert(0, ROOT)
    import torch
    rt = importlib.import_module("tpp-mlir_amd").get_runtime()
    torch.cuda.set_device(0)
    rt.set_async(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say("# skinny-batch f32 layer chains (xsmm_hip_set_chain_skinny_f32): call by call against one launch; one process, one GPU")
    say("# box: %s, %d CUs; three layers, bias + relu; command: %s" % (props.name, props.multi_processor_count, " ".join(sys.argv)))
    if not args.rule_only:
        say("# per side: %d steps between two events, %d alternating rounds; us per step: median [min .. max]; a = calls under skinny_f32(1) + skinny_f32_split(1) (the baseline), "
            "b = calls, every switch off; 16 / 32 / 64 = set_chain_skinny_f32; (G, BN, waves) of the launch; wins = rounds faster than a" % (args.iters, args.rounds))
    if args.chain_split:
        say("# --chain-split: %d steps between two events, %d alternating rounds; us per step: median [min .. max]; a = calls under skinny_f32(1) + skinny_f32_split(1) on the PARENT's "
            "library (a child process per round); uBN = set_chain_skinny_f32(BN) unsplit; BN/P = + set_chain_skinny_f32_split(P); (G, BN, waves); wins = rounds faster than a" % (args.iters, args.rounds))
        chain_split_ab(args, rt, say)
    rule = []
    for k0, ns in ([] if args.chain_split else CHAINS):
        for m in MS:
            s = Step(rt, m, k0, ns)
            set_side(rt, "rule")  # what mode 1 does with the row: one step
            before = rt.chain_skinny_f32_stats()[0]
            s.run()
            rt.synchronize()
            st = rt.chain_skinny_f32_stats()
            rule.append("%-40s %s" % (name(m, k0, ns), "G %d BN %d waves %d" % st[1:4] if st[0] > before and s.fused else "calls"))
            set_side(rt, "b")
            if args.rule_only:
                continue
            sides = [x for x in SIDES if not isinstance(x, int) or min(ns) >= x]
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.1:  # clocks up, every side warm
                for x in sides:
                    set_side(rt, x)
                    s.timed(args.iters)
            us, how = {x: [] for x in sides}, {}
            for _ in range(args.rounds):
                for x in sides:
                    set_side(rt, x)
                    before = rt.chain_skinny_f32_stats()[0]
                    t, fused = s.timed(args.iters)
                    st = rt.chain_skinny_f32_stats()
                    how[x] = "G %d BN %d W %d" % st[1:4] if st[0] > before and fused else "calls"
                    us[x].append(t)
            set_side(rt, "b")
            say(name(m, k0, ns))
            for x in sides:
                wins = sum(b < a for a, b in zip(us["a"], us[x]))
                say("    %-5s %8.2f [%8.2f .. %8.2f]  %-16s %s   rounds: %s" % (x, statistics.median(us[x]), min(us[x]), max(us[x]), how[x],
                    "" if x in ("a", "b") else "%+6.1f %% against a, wins %d / %d" % (100.0 * (statistics.median(us[x]) - statistics.median(us["a"])) / statistics.median(us["a"]), wins, args.rounds),
                    " ".join("%.2f" % v for v in us[x])))
    if not args.chain_split:
        say("# what set_chain_skinny_f32(1) does with each row (gemm_plan.cpp plan_chain_skinny_f32)")
    for r in rule:
        say("    " + r)
    if args.parent_root and not args.rule_only:
        say("# controls against the parent commit's library: child processes - the parent's, this tree's with every switch as it starts - alternating (and alternating in who goes first), %d each" % args.rounds)
        order = [("this tree", ROOT), ("parent", os.path.abspath(args.parent_root))]
        got = {who: {} for who, _ in order}
        for pair in range(args.rounds):
            for who, root in (order if pair % 2 == 0 else order[::-1]):  # (the first child of a round finds the clocks lower)
                for what, (t_us, _) in run_child(args, "--child-control", root).items():
                    got[who].setdefault(what, []).append(t_us)
        for what, a in got["parent"].items():
            b = got["this tree"][what]
            say("%-52s parent %8.2f [%8.2f .. %8.2f] | this tree %8.2f [%8.2f .. %8.2f] %+5.1f %% %s" % (
                what, statistics.median(a), min(a), max(a), statistics.median(b), min(b), max(b), 100.0 * (statistics.median(b) - statistics.median(a)) / statistics.median(a),
                "inside the parent's spread" if min(a) <= statistics.median(b) <= max(a) else "OUTSIDE the parent's spread"))
    say("# not measured: other CU counts, several ranks, layers between the measured sizes" + (
        ", P beyond 4, BN 64, the bf16 twin (not built)" if args.chain_split else ", a K split across workgroups inside the chain (--chain-split)"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
