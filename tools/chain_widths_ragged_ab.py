#!/usr/bin/env python3
"""A/B of the ragged mixed-width bf16 layer chain (xsmm_hip_set_chain_widths_ragged) on one GPU: a rank's MLP step - bf16,
VNNI-2 weights, bias + relu, device-resident operands, asynchronous mode - through xsmm_hip_fused_brgemm_chain_invoke, timed with events
around --iters steps. Every row is warmed up on both sides, then runs --pairs alternating pairs
    off: the switch off, the three single-call switches on (set_edge_tiles(2), set_edge_k_bf16(1), set_edge_k8_bf16(1)): call by call - the
         parent commit's behaviour
    on:  the same + set_chain_widths_ragged(1): one launch, where the rule takes the chain
and reports every pair, then median, min and max of each side. A row counts as FASTER if every pair is faster or the median gain exceeds
the spread (max - min) of the row's switch-off runs; SLOWER the same way round; else "no difference shown". A row slower as one launch in
the majority of its pairs asks for a gate in plan_chain_widths_ragged. --force-tile T measures the rows with set_edge_tiles(20 + T): the
rule's gate does not apply under a forcing edge-tile mode, which is how a gated row is measured as one launch.
Controls (unchanged launches; the new switch off against on in this process): the equal-width 1024- and 4096-row chains (the plain chain),
the funnel 1024 rows x [1024, 512, 256, 128] under set_chain_widths(1) (mode 9), [1000] * 4 at 1000 rows under set_chain_ragged(1)
(mode 8) - and, with --parent-root DIR (a checkout of the parent commit with its library built), the same four on the parent's library in
child processes that alternate with child processes on this tree's.
    python tools/chain_widths_ragged_ab.py --out profiles/chain_widths_ragged_ab.txt [--parent-root DIR]"""
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
    (1024, [784, 512, 256, 128]),
    (1000, [784, 512, 256, 128]),
    (1000, [1024, 512, 256, 128]),
    (512, [784, 256, 64, 256, 784]),
    (1000, [1000, 500, 250]),
    (1000, [1000, 504, 248]),
    (200, [200, 136, 72, 200]),
    (1000, [1000, 2000, 1000]),
]
# rows, layer widths, the switches of the control besides the new one: "plain" none, "widths" set_chain_widths(1), "ragged" singles + set_chain_ragged(1)
CONTROLS = [(1024, [1024] * 4, "plain"), (4096, [1024] * 4, "plain"), (1024, [1024, 512, 256, 128], "widths"), (1000, [1000] * 4, "ragged")]


def name(rows, layers, kind=None):
    return "%d rows x %s%s" % (rows, layers, {None: "", "plain": " (the plain chain)", "widths": " (mode 9, set_chain_widths)", "ragged": " (mode 8, set_chain_ragged)"}[kind])


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


def singles(rt, on, tile=-1):
    rt.set_edge_tiles((20 + tile if tile >= 0 else 2) if on else 0), rt.set_edge_k_bf16((20 + tile if tile >= 0 else 1) if on else 0)
    rt.set_edge_k8_bf16((20 + tile if tile >= 0 else 1) if on else 0)


def control_switches(rt, kind, on):
    if kind == "widths":
        rt.set_chain_widths(1 if on else 0)
    if kind == "ragged":
        singles(rt, on)
        rt.set_chain_ragged(1 if on else 0)


def verdict(offs, ons):
    med0, med1, spread = statistics.median(offs), statistics.median(ons), max(offs) - min(offs)
    if all(b < a for a, b in zip(offs, ons)) or (med0 - med1 > spread and med1 < med0):
        return "FASTER"
    if all(b > a for a, b in zip(offs, ons)) or (med1 - med0 > spread and med1 > med0):
        return "SLOWER"
    return "no difference shown"


def child_control(root, iters):
    """the controls on the library of the tree at `root`, each under its own switches: one JSON line of us per step"""
    sys.path.insert(0, root)
    pkg = importlib.import_module("tpp-mlir_amd")
    rt = pkg.get_runtime()
    rt.set_async(True)
    out = {}
    for rows, layers, kind in CONTROLS:
        s = Step(pkg, rt, rows, layers)
        control_switches(rt, kind, True)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:
            s.timed(iters)
        us, fused = s.timed(iters)
        control_switches(rt, kind, False)
        out[name(rows, layers, kind)] = (us, fused)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--force-tile", type=int, default=-1, help="measure the rows under set_edge_tiles / _edge_k_bf16 / _edge_k8_bf16(20 + T): no gate applies")
    ap.add_argument("--only", default="", help="comma-separated indices into the row list (default: all)")
    ap.add_argument("--no-controls", action="store_true")
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
    say("# ragged mixed-width bf16 layer chains (xsmm_hip_set_chain_widths_ragged): call by call under the three single-call switches against one launch; one process, one GPU")
    say("# box: %s, %d CUs; VNNI-2 B, bias + relu; command: %s" % (props.name, props.multi_processor_count, " ".join(sys.argv)))
    say("# per side: %d steps between two events, %d alternating pairs; us per step: median [min .. max]; launch: tile rows x tile columns, variant; then every pair off/on" % (args.iters, args.pairs))

    def ab(rows, layers, kind=None):
        s = Step(pkg, rt, rows, layers)

        def side(on):
            if kind is None:
                singles(rt, True, args.force_tile)
            else:
                control_switches(rt, kind, True)
            rt.set_chain_widths_ragged(on)
            r = s.timed(args.iters)
            rt.set_chain_widths_ragged(0)
            singles(rt, False), control_switches(rt, kind, False)
            return r
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:  # clocks up, both sides warm
            side(0), side(1)
        before = rt.chain_widths_ragged_stats()[0]
        offs, ons, fused = [], [], {}
        for _ in range(args.pairs):
            a, fused[0] = side(0)
            b, fused[1] = side(1)
            offs.append(a), ons.append(b)
        st = rt.chain_widths_ragged_stats()
        launch = "%d x %d, variant %d" % st[1:] if st[0] > before else "no ragged mixed-width launch"
        med0, med1 = statistics.median(offs), statistics.median(ons)
        say("%-52s off %8.2f [%8.2f .. %8.2f] %-12s | on %8.2f [%8.2f .. %8.2f] %-12s (%s) | %+6.1f %%  %s  pairs faster %d / %d | pairs %s" % (
            name(rows, layers, kind), med0, min(offs), max(offs), "one launch" if fused[0] else "call by call", med1, min(ons), max(ons), "one launch" if fused[1] else "call by call",
            launch, 100.0 * (med1 - med0) / med0, verdict(offs, ons) if kind is None else "(control: the same launch on both sides) " + verdict(offs, ons),
            sum(b < a for a, b in zip(offs, ons)), len(offs), " ".join("%.2f/%.2f" % p for p in zip(offs, ons))))

    only = [int(x) for x in args.only.split(",")] if args.only else range(len(ROWS))
    for i in only:
        try:
            ab(*ROWS[i])
        except Exception as e:  # (a shape the MLP itself does not take: on record, the other rows go on)
            say("%-52s not measured: %s" % (name(*ROWS[i]), str(e).replace("\n", " ")[:200]))
    if not args.no_controls:
        say("# controls: unchanged launches, the new switch off against on, each under its own switches")
        for rows, layers, kind in CONTROLS:
            ab(rows, layers, kind)
    if args.parent_root:
        say("# controls against the parent commit's library: child processes, this tree and the parent's alternating (and alternating in who goes first), %d each; the new switch off" % args.pairs)
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
        for rows, layers, kind in CONTROLS:
            what = name(rows, layers, kind)
            a, b = [u for u, _ in got["parent"].get(what, [])], [u for u, _ in got["this tree"].get(what, [])]
            if a and b:
                say("%-52s parent %8.2f [%8.2f .. %8.2f] | this tree %8.2f [%8.2f .. %8.2f] | %+6.1f %%  %s | parent %s | this tree %s" % (
                    what, statistics.median(a), min(a), max(a), statistics.median(b), min(b), max(b),
                    100.0 * (statistics.median(b) - statistics.median(a)) / statistics.median(a), verdict(a, b), " ".join("%.2f" % v for v in a), " ".join("%.2f" % v for v in b)))
    say("# not measured: flat and VNNI-4 B, other CU counts, several ranks; this mode in column rounds, a run-ahead across a seam and two chunks per barrier (never built)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
