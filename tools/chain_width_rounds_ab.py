#!/usr/bin/env python3
"""A/B of column rounds of mixed-width bf16 layer chains (xsmm_hip_set_chain_width_rounds) on one GPU: a rank's MLP step -
bf16, VNNI-2 weights, bias + relu, device-resident operands, asynchronous mode - through xsmm_hip_fused_brgemm_chain_invoke, timed with
events around --iters steps. Every row is warmed up on every side, then runs --pairs alternating pairs
    off: every chain switch off: call by call - the baseline of the row, in the same session and the same binary
    on:  set_chain_width_rounds(1) (or 1000 + W where the row says so): one launch on m / BM x W workgroups, unless the rule gates it
and reports the median, min and max of each side and every pair. For the row the one-round rule takes today, set_chain_widths(1) alone is
measured in --pairs runs of its own BEHIND the pairs (as a third alternating side it made the call-by-call side that followed it about
1 us faster than the same side anywhere else) and compared with the row's switch-off median. A row counts as FASTER if every pair is faster or the median gain exceeds
the spread (max - min) of the row's switch-off runs; SLOWER the same way round; else "no difference shown".
Rows with tile = t are dispatched under force_variant(20 + t): the calls and the launch share that tile (the forced-W rows: W moves, the
tile does not).
Controls: the equal-width 1024-wide chain at 1024 and 4096 rows, switch off against switch on (the plain chain kernel on both sides) - and,
with --parent-root DIR (a checkout of the parent commit with its library built), the same two chains and the funnel under
set_chain_widths(1) on the parent's library in child processes that alternate with child processes on this tree's, switch off and on.
    python tools/chain_width_rounds_ab.py --out profiles/chain_width_rounds_ab.txt [--parent-root DIR]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rows, layer widths, forced tile (None: the planner's), forced W (None: mode 1)
ROWS = [
    (256, [1024, 4096, 1024], None, None),
    (1024, [1024, 4096, 1024], None, None),
    (2048, [1024, 4096, 1024], None, None),
    (4096, [1024, 4096, 1024], None, None),
    (2048, [1024, 2048, 1024], None, None),
    (1024, [1024, 2048, 1024, 2048, 1024], None, None),
    (1024, [1024, 512, 256, 128], None, None),
    (1024, [1024, 512, 256, 128], None, 4),
    (1024, [1024, 4096, 1024], 1, None),
    (1024, [1024, 4096, 1024], 1, 8),
    (1024, [1024, 4096, 1024], 1, 16),
]
CONTROLS = [(1024, [1024] * 4), (4096, [1024] * 4)]
FUNNEL = (1024, [1024, 512, 256, 128])
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]


def name(rows, layers, tile=None, w=None):
    return "%d rows x %s%s%s" % (rows, layers, "" if tile is None else " on %dx%d" % TILE[tile], "" if w is None else " W = %d" % w)


class Step:
    def __init__(self, pkg, rt, rows, layers, tile=None):
        import torch
        self.rt, self.torch = rt, torch
        self.spec = pkg.MlpSpec(batch=rows, layers=layers)
        rt.force_variant(-1 if tile is None else 20 + tile)
        try:
            self.mlp = pkg.ShardedMlp(self.spec, 0, 1, rt)
            g = torch.Generator().manual_seed(7)
            self.x = (torch.randn(rows, layers[0], generator=g) * 0.5).to(torch.bfloat16).cuda()
            self.w = [(torch.randn(k // 2, n, 2, generator=g) * 0.05).to(torch.bfloat16).cuda() for k, n in zip(layers[:-1], layers[1:])]
            self.b = [(torch.randn(n, generator=g) * 0.1).to(torch.bfloat16).cuda() for n in layers[1:]]
            self.acts = [torch.zeros(rows, n, dtype=torch.bfloat16, device="cuda") for n in layers[1:]]
            self.run()  # (the descriptors are dispatched by now, under the forced tile)
            rt.synchronize()
        finally:
            rt.force_variant(-1)

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


def child_control(root, iters, switch):
    """the two equal-width chains, and the funnel under set_chain_widths(1), on the library of the tree at `root`; `switch`: this tree's
    column-round switch (the parent has none). One JSON line of us per step"""
    sys.path.insert(0, root)
    pkg = importlib.import_module("tpp-mlir_amd")
    rt = pkg.get_runtime()
    rt.set_async(True)
    if switch and hasattr(rt, "set_chain_width_rounds"):
        rt.set_chain_width_rounds(switch)
    out = {}
    for rows, layers in CONTROLS + [FUNNEL]:
        rt.set_chain_widths(1 if (rows, layers) == FUNNEL else 0)
        s = Step(pkg, rt, rows, layers)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:
            s.timed(iters)
        out[name(rows, layers)] = s.timed(iters)
    rt.set_chain_widths(0)
    if hasattr(rt, "set_chain_width_rounds"):
        rt.set_chain_width_rounds(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--child-control", default="", help="(internal) run the controls on the tree at this root and print JSON")
    ap.add_argument("--child-switch", type=int, default=0, help="(internal) the column-round switch of the child")
    args = ap.parse_args()
    if args.child_control:
        return child_control(args.child_control, args.iters, args.child_switch)
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
    say("# column rounds of mixed-width bf16 layer chains (xsmm_hip_set_chain_width_rounds): call by call (every chain switch off) against one launch; one process, one GPU")
    say("# box: %s, %d CUs; VNNI-2 B, bias + relu; command: %s" % (props.name, props.multi_processor_count, " ".join(sys.argv)))
    say("# per side: %d steps between two events, %d alternating pairs; us per step: median [min .. max]; launch: row blocks x W workgroup columns, variant; every pair: off/on" % (args.iters, args.pairs))

    def ab(rows, layers, tile=None, w=None, control=False, third=False):
        s = Step(pkg, rt, rows, layers, tile)
        mode = 1 if w is None else 1000 + w

        def side(which):
            rt.set_chain_width_rounds(mode if which == 1 else 0)
            rt.set_chain_widths(1 if which == 2 else 0)
            r = s.timed(args.iters)
            rt.set_chain_width_rounds(0), rt.set_chain_widths(0)
            return r
        sides = (0, 1)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:  # clocks up, every side warm
            for x in sides:
                side(x)
        before = rt.chain_width_rounds_stats()[0]
        us, fused = {x: [] for x in sides}, {}
        for _ in range(args.pairs):
            for x in sides:
                a, fused[x] = side(x)
                us[x].append(a)
        st = rt.chain_width_rounds_stats()
        launch = "%d x %d, variant %d" % st[1:] if st[0] > before else "no column-round launch"
        med = {x: statistics.median(us[x]) for x in sides}
        how = lambda x: "one launch" if fused[x] else "call by call"
        text = "%-58s off %8.2f [%8.2f .. %8.2f] %-12s | on %8.2f [%8.2f .. %8.2f] %-12s (%s%s) | %+6.1f %%  %s  pairs faster %d / %d" % (
            name(rows, layers, tile, w), med[0], min(us[0]), max(us[0]), how(0), med[1], min(us[1]), max(us[1]), how(1), launch, "", 100.0 * (med[1] - med[0]) / med[0],
            verdict(us[0], us[1]) if not control else "(control: the same kernel on both sides) " + verdict(us[0], us[1]), sum(b < a for a, b in zip(us[0], us[1])), len(us[0]))
        if third:
            side(2)
            us[2] = [side(2)[0] for _ in range(args.pairs)]
            fused[2] = bool(s.mlp.last_step_fused)
            med[2] = statistics.median(us[2])
            text += " | one round (set_chain_widths) %8.2f [%8.2f .. %8.2f] %-12s %+6.1f %%" % (med[2], min(us[2]), max(us[2]), how(2), 100.0 * (med[2] - med[0]) / med[0])
        say(text)
        say("#     pairs: " + "  ".join("/".join("%.2f" % us[x][i] for x in sides) for i in range(args.pairs)) + ("   one round: " + " ".join("%.2f" % v for v in us[2]) if third else ""))

    for rows, layers, tile, w in ROWS:
        ab(rows, layers, tile, w, third=(rows, layers) == FUNNEL and w is None)
    say("# controls: equal-width chains, the switch off against the switch on")
    for rows, layers in CONTROLS:
        ab(rows, layers, control=True)
    if args.parent_root:
        say("# controls against the parent commit's library: child processes - the parent's, this tree's with the switch off, this tree's with the switch at 1 - alternating (and alternating in who goes first), %d each; the funnel under set_chain_widths(1)" % args.pairs)
        order = [("this tree, switch off", ROOT, 0), ("parent", os.path.abspath(args.parent_root), 0), ("this tree, switch on", ROOT, 1)]
        got = {who: {} for who, _, _ in order}
        for pair in range(args.pairs):
            for who, root, sw in (order if pair % 2 == 0 else order[::-1]):  # (who goes first alternates: the first child of a pair finds the clocks lower)
                env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_") and k != "TPP_XSMM_LIBRARY"}
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-control", root, "--iters", str(args.iters), "--child-switch", str(sw)],
                                   capture_output=True, text=True, env=env, timeout=300)
                if p.returncode != 0:
                    say("# child on %s failed: %s" % (who, p.stderr[-400:].replace("\n", " ")))
                    continue
                for what, (t_us, fused) in json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1]).items():
                    got[who].setdefault(what, []).append((t_us, fused))
        for rows, layers in CONTROLS + [FUNNEL]:
            what = name(rows, layers)
            a = [u for u, _ in got["parent"].get(what, [])]
            if not a:
                continue
            text = "%-58s parent %8.2f [%8.2f .. %8.2f]" % (what, statistics.median(a), min(a), max(a))
            for who in ("this tree, switch off", "this tree, switch on"):
                b = [u for u, _ in got[who].get(what, [])]
                if b:
                    inside = min(a) <= statistics.median(b) <= max(a)
                    text += " | %s %8.2f [%8.2f .. %8.2f] %+5.1f %% %s" % (who, statistics.median(b), min(b), max(b), 100.0 * (statistics.median(b) - statistics.median(a)) / statistics.median(a),
                                                                         "inside the parent's spread" if inside else verdict(a, b))
            say(text)
    say("# not measured: flat and VNNI-4 B, other CU counts, several ranks; the A loaders never run ahead - the one form built")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
