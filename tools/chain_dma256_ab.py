#!/usr/bin/env python3
"""A/B of layer chains on the 256x256 bf16 tile (xsmm_hip_set_chain_dma256) on one GPU: a rank's MLP step - bf16, bias + relu,
device-resident operands, asynchronous mode, whole-layer calls in 64-k batch elements - through xsmm_hip_fused_brgemm_chain_invoke, timed
with events around --iters steps. Every row is warmed up on every side, then runs --pairs alternating pairs
    off: EVERY chain switch off: call by call - the baseline of the row, in the same session and the same binary
    on:  set_chain_dma256(<the row's mode>): one launch of brgemm_bf16_dma256_chain, unless the rule refuses or gates it
and reports the median, min and max of each side and every pair. A row counts as FASTER if every pair is faster or the median gain exceeds
the spread (max - min) of the row's switch-off runs; SLOWER the same way round; else "no difference shown". The flat and VNNI-4 rows run
under set_dma256_images(1) on both sides (what puts their separate calls on the tile). Beside the 8192- and 16384-row rows: the same chain
under set_chain_rounds(1000 + G) on the 128x128 loader-wave tile, in --pairs runs of its own behind the pairs.
Controls: the plain chain at 1024 and 4096 rows and the single call 4096 x 4096 x 1024 on brgemm_bf16_dma256, switch off against switch on
(the same kernels on both sides) - and, with --parent-root DIR (a checkout of the parent commit with its library built), the same three on
the parent's library in child processes that alternate with child processes on this tree's, switch off and on.
    python tools/chain_dma256_ab.py --out profiles/chain_dma256_ab.txt [--parent-root DIR]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = 2

# rows, width, B image (2 VNNI-2, 0 flat, 4 VNNI-4), the row's mode, G of the chain_rounds side (None: none)
ROWS = [
    (8192, 1024, 2, 2, 32),
    (16384, 1024, 2, 1, 32),
    (32768, 1024, 2, 1, None),
    (4096, 4096, 2, 1, None),
    (16384, 1024, 0, 1, None),
    (16384, 1024, 4, 1, None),
]
CONTROLS = [(1024, 1024), (4096, 1024)]
IMAGE = {2: "VNNI-2", 0: "flat", 4: "VNNI-4"}


def name(rows, width, image=2, layers=3):
    return "%d rows x %d layers of %d, %s" % (rows, layers, width, IMAGE[image])


class Step:
    """`layers` whole-layer calls of rows x width (k = width in 64-k batch elements), as tpp-mlir_amd/mlp.py dispatches them, with B image `image`"""

    def __init__(self, rt, rows, width, image=2, layers=3):
        import torch
        self.rt, self.torch, self.fused = rt, torch, False
        old = rt.set_vnni_factor(image) if image else None
        try:
            flags = 4 | (2048 if image else 0)
            self.handles = [rt.fused_brgemm_dispatch(BF16, rows, width, 64, width, width, width, 64, 64 * width, flags, 0, 5, 4, 1) for _ in range(layers)]
        finally:
            if image:
                rt.set_vnni_factor(old)
        g = torch.Generator().manual_seed(7)
        self.x = (torch.randn(rows, width, generator=g) * 0.5).to(torch.bfloat16).cuda()
        self.w = [(torch.randn(width, width, generator=g) * 0.05).to(torch.bfloat16).cuda() for _ in range(layers)]
        self.b = [(torch.randn(width, generator=g) * 0.1).to(torch.bfloat16).cuda() for _ in range(layers)]
        self.acts = [torch.zeros(rows, width, dtype=torch.bfloat16, device="cuda") for _ in range(layers)]
        self.br = width // 64
        self.run()
        rt.synchronize()

    def run(self):
        cur, calls = self.x, []
        for l, h in enumerate(self.handles):
            calls.append((h, cur, 0, self.w[l], 0, self.acts[l], 0, self.b[l], 0, self.br))
            cur = self.acts[l]
        self.fused = bool(self.rt.fused_brgemm_chain(BF16, calls))

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
    """the single call 4096 x 4096 x 1024 (VNNI-2, bias + relu): brgemm_bf16_dma256 by the planner's rule"""

    def __init__(self, rt):
        import torch
        self.rt, self.torch, self.fused = rt, torch, False
        self.h = rt.fused_brgemm_dispatch(BF16, 4096, 4096, 64, 1024, 4096, 4096, 64, 64 * 4096, 4 | 2048, 0, 5, 4, 1)
        g = torch.Generator().manual_seed(7)
        self.x = (torch.randn(4096, 1024, generator=g) * 0.5).to(torch.bfloat16).cuda()
        self.w = (torch.randn(1024, 4096, generator=g) * 0.05).to(torch.bfloat16).cuda()
        self.b = (torch.randn(4096, generator=g) * 0.1).to(torch.bfloat16).cuda()
        self.c = torch.zeros(4096, 4096, dtype=torch.bfloat16, device="cuda")
        self.kernel = rt.kernel_name(self.h)

    def run(self):
        self.rt.fused_brgemm(BF16, self.h, self.x, 0, self.w, 0, self.c, 0, self.b, 0, 16)

    timed = Step.timed


def verdict(offs, ons):
    med0, med1, spread = statistics.median(offs), statistics.median(ons), max(offs) - min(offs)
    if all(b < a for a, b in zip(offs, ons)) or (med0 - med1 > spread and med1 < med0):
        return "FASTER"
    if all(b > a for a, b in zip(offs, ons)) or (med1 - med0 > spread and med1 > med0):
        return "SLOWER"
    return "no difference shown"


def controls(rt):
    return [(name(r, w), Step(rt, r, w)) for r, w in CONTROLS] + [("single call 4096 x 4096 x 1024", Single(rt))]


def child_control(root, iters, switch):
    """the controls on the library of the tree at `root`; `switch`: this tree's switch (the parent has none). One JSON line of us per step"""
    sys.path.insert(0, root)
    pkg = importlib.import_module("tpp-mlir_amd")
    rt = pkg.get_runtime()
    rt.set_async(True)
    if switch and hasattr(rt, "set_chain_dma256"):
        rt.set_chain_dma256(switch)
    out = {}
    for what, s in controls(rt):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:
            s.timed(iters)
        out[what] = s.timed(iters)
    if hasattr(rt, "set_chain_dma256"):
        rt.set_chain_dma256(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--child-control", default="", help="(internal) run the controls on the tree at this root and print JSON")
    ap.add_argument("--child-switch", type=int, default=0, help="(internal) the switch of the child")
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
    say("# layer chains on the 256x256 bf16 tile (xsmm_hip_set_chain_dma256): call by call (every chain switch off) against one launch; one process, one GPU")
    say("# box: %s, %d CUs; bias + relu; command: %s" % (props.name, props.multi_processor_count, " ".join(sys.argv)))
    say("# per side: %d steps between two events, %d alternating pairs; us per step: median [min .. max]; launch: G row groups x rounds, B image; every pair: off/on" % (args.iters, args.pairs))

    def ab(what, s, mode, images=0, rounds_g=None, control=False):
        def side(which):
            rt.set_dma256_images(images)
            rt.set_chain_dma256(mode if which == 1 else 0)
            rt.set_chain_rounds(1000 + rounds_g if which == 2 else 0)
            r = s.timed(args.iters)
            rt.set_chain_dma256(0), rt.set_chain_rounds(0), rt.set_dma256_images(0)
            return r
        sides = (0, 1)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:  # clocks up, every side warm
            for x in sides:
                side(x)
        before = rt.chain_dma256_stats()[0]
        us, fused = {x: [] for x in sides}, {}
        for _ in range(args.pairs):
            for x in sides:
                a, fused[x] = side(x)
                us[x].append(a)
        st = rt.chain_dma256_stats()
        launch = "G = %d, R = %d, image %d" % st[1:] if st[0] > before else "no launch on the 256x256 tile"
        med = {x: statistics.median(us[x]) for x in sides}
        how = lambda x: "one launch" if fused[x] else "call by call"
        text = "%-44s mode %-4d off %8.2f [%8.2f .. %8.2f] %-12s | on %8.2f [%8.2f .. %8.2f] %-12s (%s) | %+6.1f %%  %s  pairs faster %d / %d" % (
            what, mode, med[0], min(us[0]), max(us[0]), how(0), med[1], min(us[1]), max(us[1]), how(1), launch, 100.0 * (med[1] - med[0]) / med[0],
            ("(control: the same kernels on both sides) " if control else "") + verdict(us[0], us[1]), sum(b < a for a, b in zip(us[0], us[1])), len(us[0]))
        if rounds_g:
            side(2)
            us[2] = [side(2)[0] for _ in range(args.pairs)]
            st2 = rt.chain_rounds_stats()
            text += " | set_chain_rounds(%d) on 128x128 %8.2f [%8.2f .. %8.2f] (G = %d, R = %d) %+6.1f %%" % (1000 + rounds_g, statistics.median(us[2]), min(us[2]), max(us[2]), st2[1], st2[2],
                                                                                                     100.0 * (statistics.median(us[2]) - med[0]) / med[0])
        say(text)
        say("#     pairs: " + "  ".join("/".join("%.2f" % us[x][i] for x in sides) for i in range(args.pairs)) + ("   chain_rounds: " + " ".join("%.2f" % v for v in us[2]) if rounds_g else ""))

    for rows, width, image, mode, rounds_g in ROWS:
        ab(name(rows, width, image), Step(rt, rows, width, image), mode, images=1 if image != 2 else 0, rounds_g=rounds_g)
    say("# controls: the switch off against the switch on (mode 1) where it takes nothing - the plain chain, a single call on %s" % Single(rt).kernel)
    for what, s in controls(rt):
        ab(what, s, 1, control=True)
    if args.parent_root:
        say("# controls against the parent commit's library: child processes - the parent's, this tree's with the switch off, this tree's with the switch at 1 - alternating (and alternating in who goes first), %d each" % args.pairs)
        order = [("this tree, switch off", ROOT, 0), ("parent", os.path.abspath(args.parent_root), 0), ("this tree, switch on", ROOT, 1)]
        got = {who: {} for who, _, _ in order}
        for pair in range(args.pairs):
            for who, root, sw in (order if pair % 2 == 0 else order[::-1]):  # (the first child of a pair finds the clocks lower)
                env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_") and k != "TPP_XSMM_LIBRARY"}
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-control", root, "--iters", str(args.iters), "--child-switch", str(sw)],
                                   capture_output=True, text=True, env=env, timeout=300)
                if p.returncode != 0:
                    say("# child on %s failed: %s" % (who, p.stderr[-400:].replace("\n", " ")))
                    continue
                for what, (t_us, fused) in json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1]).items():
                    got[who].setdefault(what, []).append((t_us, fused))
        for what in list(got["parent"]):
            a = [u for u, _ in got["parent"].get(what, [])]
            text = "%-44s parent %8.2f [%8.2f .. %8.2f]" % (what, statistics.median(a), min(a), max(a))
            for who in ("this tree, switch off", "this tree, switch on"):
                b = [u for u, _ in got[who].get(what, [])]
                if b:
                    inside = min(a) <= statistics.median(b) <= max(a)
                    text += " | %s %8.2f [%8.2f .. %8.2f] %+5.1f %% %s" % (who, statistics.median(b), min(b), max(b), 100.0 * (statistics.median(b) - statistics.median(a)) / statistics.median(a),
                                                                         "inside the parent's spread" if inside else verdict(a, b))
            say(text)
    say("# not measured: other CU counts, several ranks, beta 1 (not a chain), K other than these, sc1 on the later layers' A loads only, B run-ahead across a seam")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
