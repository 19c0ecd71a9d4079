#!/usr/bin/env python3
"""A/B of skinny-batch layer chains (xsmm_hip_set_chain_skinny) on one GPU: a rank's MLP step with 1 .. 31 rows - bf16, bias +
relu, device-resident operands, asynchronous mode, whole-layer calls as tpp-mlir_amd/mlp.py dispatches them (64-k batch elements where 64
divides k) - through xsmm_hip_fused_brgemm_chain_invoke, timed with events around --iters steps. Every row is warmed up on every side, then
runs --rounds alternating rounds of
    a     call by call under set_skinny_bf16(1) and set_skinny_split(1): the best existing form, THE BASELINE
    b     call by call with every switch off (the generic kernel)
    16 / 32 / 64   one launch under set_chain_skinny(BN), where the image has an instance and every layer is wide enough
    rule  set_chain_skinny(1): one launch on the rule's BN, or call by call where the rule gates or refuses
and reports the median [min .. max] of each side in us per step and, per one-launch side, in how many rounds it beat (a). Mode 1 may take
exactly the (row, BN) that beat (a) in EVERY round.
Controls, with --parent-root DIR (a checkout of the parent commit with its library built): child processes on the parent's library
alternate with child processes on this tree's - the 4096-row plain chain of three 1024-wide layers and the single call 1024 x 1024 x 1024
with the switch off and on (this tree), and every row call by call with every switch off.
    python tools/chain_skinny_ab.py --out profiles/chain_skinny_ab.txt [--parent-root DIR]"""
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
MS = [1, 8, 16, 31]
# (the input's width, every layer's n), B images (2 VNNI-2, 0 flat, 4 VNNI-4)
CHAINS = [((4096, [4096] * 3), (2, 0, 4)), ((1024, [1024] * 3), (2,)), ((1000, [1000] * 3), (2,)), ((4096, [4096, 11008, 4096]), (2,)), ((784, [512, 256, 128]), (2,))]
IMAGE = {2: "VNNI-2", 0: "flat", 4: "VNNI-4"}
SIDES = ["a", "b", 16, 32, 64, "rule"]


def name(m, k0, ns, image):
    return "m %2d  %d -> %s, %s" % (m, k0, " -> ".join(str(n) for n in ns), IMAGE[image])


class Step:
    """whole-layer calls of m rows: layer l is [m x k_l] @ [k_l x ns[l]], k_l in 64-k batch elements where 64 divides it, B image `image`"""

    def __init__(self, rt, m, k0, ns, image=2):
        import torch
        self.rt, self.torch, self.fused = rt, torch, False
        old = rt.set_vnni_factor(image) if image else None
        ks = [k0] + list(ns[:-1])
        self.brs = [k // 64 if k % 64 == 0 else 1 for k in ks]
        try:
            flags = 4 | (2048 if image else 0)
            self.handles = [rt.fused_brgemm_dispatch(BF16, m, n, k // br, k, n, n, k // br, (k // br) * n, flags, 0, 5, 4, 1) for n, k, br in zip(ns, ks, self.brs)]
        finally:
            if image:
                rt.set_vnni_factor(old)
        g = torch.Generator().manual_seed(7)
        self.x = (torch.randn(m, k0, generator=g) * 0.5).to(torch.bfloat16).cuda()
        self.w = [(torch.randn(k, n, generator=g) * 0.05).to(torch.bfloat16).cuda() for n, k in zip(ns, ks)]
        self.b = [(torch.randn(n, generator=g) * 0.1).to(torch.bfloat16).cuda() for n in ns]
        self.acts = [torch.zeros(m, n, dtype=torch.bfloat16, device="cuda") for n in ns]
        self.run()
        rt.synchronize()

    def run(self):
        cur, calls = self.x, []
        for l, h in enumerate(self.handles):
            calls.append((h, cur, 0, self.w[l], 0, self.acts[l], 0, self.b[l], 0, self.brs[l]))
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
    """the single call 1024 x 1024 x 1024 (VNNI-2, bias + relu)"""

    def __init__(self, rt):
        import torch
        self.rt, self.torch, self.fused = rt, torch, False
        self.h = rt.fused_brgemm_dispatch(BF16, 1024, 1024, 64, 1024, 1024, 1024, 64, 64 * 1024, 4 | 2048, 0, 5, 4, 1)
        g = torch.Generator().manual_seed(7)
        self.x = (torch.randn(1024, 1024, generator=g) * 0.5).to(torch.bfloat16).cuda()
        self.w = (torch.randn(1024, 1024, generator=g) * 0.05).to(torch.bfloat16).cuda()
        self.b = (torch.randn(1024, generator=g) * 0.1).to(torch.bfloat16).cuda()
        self.c = torch.zeros(1024, 1024, dtype=torch.bfloat16, device="cuda")

    def run(self):
        self.rt.fused_brgemm(BF16, self.h, self.x, 0, self.w, 0, self.c, 0, self.b, 0, 16)

    timed = Step.timed


def set_side(rt, side):
    rt.set_skinny_bf16(1 if side == "a" else 0)
    rt.set_skinny_split(1 if side == "a" else 0)
    if hasattr(rt, "set_chain_skinny"):
        rt.set_chain_skinny(1 if side == "rule" else side if isinstance(side, int) else 0)


def controls(rt):
    out = [("4096 rows x 3 layers of 1024, plain chain", Step(rt, 4096, 1024, [1024] * 3)), ("single call 1024 x 1024 x 1024", Single(rt))]
    for (k0, ns), images in CHAINS:
        for m in MS:
            out.append(("mode 0: " + name(m, k0, ns, 2), Step(rt, m, k0, ns, 2)))
    return out


def child_control(root, iters, switch):
    """the controls on the library of the tree at `root`; `switch`: this tree's switch (the parent has none). One JSON line of us per step"""
    sys.path.insert(0, root)
    pkg = importlib.import_module("tpp-mlir_amd")
    rt = pkg.get_runtime()
    rt.set_async(True)
    if switch and hasattr(rt, "set_chain_skinny"):
        rt.set_chain_skinny(switch)
    out = {}
    for what, s in controls(rt):
        if switch and what.startswith("mode 0"):
            continue
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:
            s.timed(iters)
        out[what] = s.timed(iters)
    if hasattr(rt, "set_chain_skinny"):
        rt.set_chain_skinny(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
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
    say("# skinny-batch layer chains (xsmm_hip_set_chain_skinny): call by call against one launch; one process, one GPU")
    say("# box: %s, %d CUs; bias + relu; command: %s" % (props.name, props.multi_processor_count, " ".join(sys.argv)))
    say("# per side: %d steps between two events, %d alternating rounds; us per step: median [min .. max]; a = calls under skinny_bf16(1) + skinny_split(1) (the baseline), "
        "b = calls, every switch off; 16 / 32 / 64 / rule = set_chain_skinny; (G, BN) of the launch; wins = rounds faster than a" % (args.iters, args.rounds))
    for (k0, ns), images in CHAINS:
        for image in images:
            for m in MS:
                s = Step(rt, m, k0, ns, image)
                sides = [x for x in SIDES if not isinstance(x, int) or (not (image == 0 and x == 16) and min(ns) >= x)]
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.1:  # clocks up, every side warm
                    for x in sides:
                        set_side(rt, x)
                        s.timed(args.iters)
                us, how = {x: [] for x in sides}, {}
                for _ in range(args.rounds):
                    for x in sides:
                        set_side(rt, x)
                        before = rt.chain_skinny_stats()[0]
                        t, fused = s.timed(args.iters)
                        st = rt.chain_skinny_stats()
                        how[x] = "G %d BN %d" % st[1:3] if st[0] > before and fused else "calls"
                        us[x].append(t)
                set_side(rt, "b")
                say(name(m, k0, ns, image))
                for x in sides:
                    wins = sum(b < a for a, b in zip(us["a"], us[x]))
                    say("    %-5s %8.2f [%8.2f .. %8.2f]  %-12s %s   rounds: %s" % (x, statistics.median(us[x]), min(us[x]), max(us[x]), how[x],
                        "" if x in ("a", "b") else "%+6.1f %% against a, wins %d / %d" % (100.0 * (statistics.median(us[x]) - statistics.median(us["a"])) / statistics.median(us["a"]), wins, args.rounds),
                        " ".join("%.2f" % v for v in us[x])))
    if args.parent_root:
        say("# controls against the parent commit's library: child processes - the parent's, this tree's with the switch off, this tree's with the switch at 1 - alternating (and alternating in who goes first), %d each" % args.rounds)
        order = [("this tree, switch off", ROOT, 0), ("parent", os.path.abspath(args.parent_root), 0), ("this tree, switch on", ROOT, 1)]
        got = {who: {} for who, _, _ in order}
        for pair in range(args.rounds):
            for who, root, sw in (order if pair % 2 == 0 else order[::-1]):  # (the first child of a round finds the clocks lower)
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
            text = "%-52s parent %8.2f [%8.2f .. %8.2f]" % (what, statistics.median(a), min(a), max(a))
            for who in ("this tree, switch off", "this tree, switch on"):
                b = [u for u, _ in got[who].get(what, [])]
                if b and not (what.startswith("mode 0") and who.endswith("on")):
                    inside = min(a) <= statistics.median(b) <= max(a)
                    text += " | %s %8.2f [%8.2f .. %8.2f] %+5.1f %% %s" % (who, statistics.median(b), min(b), max(b), 100.0 * (statistics.median(b) - statistics.median(a)) / statistics.median(a),
                                                                         "inside the parent's spread" if inside else "outside the parent's spread")
            say(text)
    say("# not measured: other CU counts, several ranks, beta 1 (not a chain), a K split across workgroups inside the chain, the launch without the weights ahead of the wait (not built)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
