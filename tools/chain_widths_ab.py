#!/usr/bin/env python3
"""A/B of the mixed-width bf16 layer chain (xsmm_hip_set_chain_widths) on one GPU: a rank's MLP step - bf16, VNNI-2 weights,
bias + relu, device-resident operands, asynchronous mode - through xsmm_hip_fused_brgemm_chain_invoke, timed with events around --iters
steps. Every row is warmed up on both sides, then runs --pairs alternating pairs
    off: the switch off: call by call (the parent's behaviour)
    on:  set_chain_widths(1): one launch
and reports median, min and max of each side. A row counts as FASTER if every pair is faster or the median gain exceeds the spread
(max - min) of the row's switch-off runs; SLOWER the same way round; else "no difference shown".
Controls: the equal-width 1024-wide chain at 1024 and 4096 rows, switch off against switch on (the plain chain kernel on both sides) - and,
with --parent-root DIR (a checkout of the parent commit with its library built), the same two chains on the parent's library in child
processes that alternate with child processes on this tree's.
    python tools/chain_widths_ab.py --out profiles/chain_widths_ab.txt [--parent-root DIR]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rows, layer widths
ROWS = [
    (1024, [1024, 4096, 1024]),
    (256, [1024, 4096, 1024]),
    (2048, [1024, 2048, 1024]),
    (1024, [1024, 512, 256, 128]),
    (1024, [1024, 2048, 1024, 2048, 1024]),
]
CONTROLS = [(1024, [1024] * 4), (4096, [1024] * 4)]


def name(rows, layers):
    return "%d rows x %s" % (rows, layers)


class Step:
    def __init__(self, pkg, rt, rows, layers):
        import torch
        self.rt, self.torch = rt, torch
        self.spec = pkg.MlpSpec(batch=rows, layers=layers)
        self.mlp = pkg.ShardedMlp(self.spec, 0, 1, rt)
        g = torch.Generator().manual_seed(7)
        self.x = (torch.randn(rows, layers[0], generator=g) * 0.5).to(torch.bfloat16).cuda()
        self.w = [(torch.randn(k // 2, n, 2, generator=g) * 0.05).to(torch.bfloat16).cuda() for k, n in zip(layers[:-1], layers[1:])]
        self.b = [(torch.randn(n, generator=g) * 0.1).to(torch.bfloat16).cuda() for n in layers[1:]]
        self.acts = [torch.zeros(rows, n, dtype=torch.bfloat16, device="cuda") for n in layers[1:]]

    def run(self):
        self.mlp.forward(self.x, self.w, self.b, self.acts)

    def timed(self, iters):
        torch = self.torch
        self.run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            self.run()
        e1.record()
        self.rt.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters, bool(self.mlp.last_step_fused)


def verdict(offs, ons):
    med0, med1, spread = statistics.median(offs), statistics.median(ons), max(offs) - min(offs)
    if all(b < a for a, b in zip(offs, ons)) or (med0 - med1 > spread and med1 < med0):
        return "FASTER"
    if all(b > a for a, b in zip(offs, ons)) or (med1 - med0 > spread and med1 > med0):
        return "SLOWER"
    return "no difference shown"


def child_control(root, iters):
    """the two equal-width chains on the library of the tree at `root`, switches as the library starts: one JSON line of us per step"""
    sys.path.insert(0, root)
    pkg = importlib.import_module("tpp-mlir_amd")
    rt = pkg.get_runtime()
    rt.set_async(True)
    out = {}
    for rows, layers in CONTROLS:
        s = Step(pkg, rt, rows, layers)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:
            s.timed(iters)
        out[name(rows, layers)] = s.timed(iters)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--child-control", default="", help="(internal) run the controls on the tree at this root and print JSON")
    args = ap.parse_args()
    if args.child_control:
        return child_control(args.child_control, args.iters)
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("tpp-mlir_amd")
    rt = pkg.get_runtime()
    torch.cuda.set_device(0)
    rt.set_async(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say("# mixed-width bf16 layer chains (xsmm_hip_set_chain_widths): call by call (the parent's behaviour) against one launch; one process, one GPU")
    say("# box: %s, %d CUs; VNNI-2 B, bias + relu; command: %s" % (props.name, props.multi_processor_count, " ".join(sys.argv)))
    say("# per side: %d steps between two events, %d alternating pairs; us per step: median [min .. max]; launch: row blocks x widest layer's column tiles, variant" % (args.iters, args.pairs))

    def ab(rows, layers, control=False):
        s = Step(pkg, rt, rows, layers)

        def side(on):
            rt.set_chain_widths(on)
            r = s.timed(args.iters)
            rt.set_chain_widths(0)
            return r
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:  # clocks up, both sides warm
            side(0), side(1)
        before = rt.chain_widths_stats()[0]
        offs, ons, fused = [], [], {}
        for _ in range(args.pairs):
            a, fused[0] = side(0)
            b, fused[1] = side(1)
            offs.append(a), ons.append(b)
        st = rt.chain_widths_stats()
        launch = "%d x %d, variant %d" % st[1:] if st[0] > before else "no mixed-width launch"
        med0, med1 = statistics.median(offs), statistics.median(ons)
        say("%-52s off %8.2f [%8.2f .. %8.2f] %-12s | on %8.2f [%8.2f .. %8.2f] %-12s (%s) | %+6.1f %%  %s  pairs faster %d / %d" % (
            name(rows, layers), med0, min(offs), max(offs), "one launch" if fused[0] else "call by call", med1, min(ons), max(ons), "one launch" if fused[1] else "call by call",
            launch, 100.0 * (med1 - med0) / med0, verdict(offs, ons) if not control else "(control: the same kernel on both sides) " + verdict(offs, ons),
            sum(b < a for a, b in zip(offs, ons)), len(offs)))

    for rows, layers in ROWS:
        ab(rows, layers)
    say("# controls: equal-width chains, the switch off against the switch on")
    for rows, layers in CONTROLS:
        ab(rows, layers, control=True)
    if args.parent_root:
        say("# controls against the parent commit's library: child processes, this tree and the parent's alternating (and alternating in who goes first), %d each; switches as the libraries start (all off)" % args.pairs)
        got = {"this tree": {}, "parent": {}}
        for pair in range(args.pairs):
            order = [("this tree", ROOT), ("parent", os.path.abspath(args.parent_root))]
            for who, root in (order if pair % 2 == 0 else order[::-1]):  # (who goes first alternates: the first child of a pair finds the clocks lower)
                env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_") and k != "TPP_XSMM_LIBRARY"}
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-control", root, "--iters", str(args.iters)], capture_output=True, text=True, env=env, timeout=300)
                if p.returncode != 0:
                    say("# child on %s failed: %s" % (who, p.stderr[-400:].replace("\n", " ")))
                    continue
                for what, (us, fused) in json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1]).items():
                    got[who].setdefault(what, []).append((us, fused))
        for rows, layers in CONTROLS:
            what = name(rows, layers)
            a, b = [u for u, _ in got["parent"].get(what, [])], [u for u, _ in got["this tree"].get(what, [])]
            if a and b:
                say("%-52s parent %8.2f [%8.2f .. %8.2f] | this tree %8.2f [%8.2f .. %8.2f] | %+6.1f %%  %s" % (
                    what, statistics.median(a), min(a), max(a), statistics.median(b), min(b), max(b),
                    100.0 * (statistics.median(b) - statistics.median(a)) / statistics.median(a), verdict(a, b)))
    say("# not measured: flat and VNNI-4 B, other CU counts, several ranks; the B loaders' run-ahead goes to the workgroup's next active layer - the one form built")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
