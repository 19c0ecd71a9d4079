#!/usr/bin/env python3
"""A/B of the skinny-batch bf16 kernel (xsmm_hip_set_skinny_bf16) on one GPU: whole-layer bf16 calls with m < 32 rows (k = 64
wide batch elements where 64 divides K, else one batch element of K; beta 0 + bias + relu) on device-resident operands in asynchronous mode,
timed with events around --iters invokes. Every row is warmed up on all its sides, then runs --pairs alternating rounds of the sides
    off   the switch off: the generic kernel (what the library does by default)
    16 / 32 / 64   xsmm_hip_set_skinny_bf16(BN): the skinny kernel on column blocks of BN (flat B: 32 and 64)
and reports per side the median, min and max in us per invoke and the bytes of B (2 K n) over the median - a skinny layer is a weight
stream - and per BN in how many rounds it was faster than `off` in the same round. Mode 1 may take a row on a BN only where that BN was
faster in EVERY round. For context (MI355X_MICROARCH: measured on this GPU family): a device copy moves 6.29 TB/s, the Infinity Cache
delivers 8.6 TB/s; B of every row but the largest fits the Infinity Cache, and back-to-back invokes re-read it from there.
--controls: calls the switch must not touch, switch off / mode 1: the 4096-row three-layer 1024-wide chain as ONE step of ShardedMlp, and a
1024 x 1024 x 1024 bf16 call. With --root <a checkout of another commit, built> the same rows run on that library (sides it has no setter
for are left out): run the two alternately for a parent / tree comparison.
--split: the K split across workgroups (xsmm_hip_set_skinny_split) instead. The sides of a row are, per BN that has an
instance of the row's B image, the skinny kernel unsplit (`16`) and with P = 2, 4, 8, 16 parts forced (`16/2` ..), and `rule`: mode 1 of
both switches. A gain is measured against the UNSPLIT skinny side of the same BN in the same round, not against the generic kernel: mode
1 of the split switch may take a row on a P only where that P was faster in EVERY round. Per row the best side is named beside the 6.29
TB/s of a copy. With --controls: the chain and the 1024^3 call, switches off / mode 1 of both, and the switch-off side of every row (on a
library without the setters the same, for a parent / tree comparison).
    python tools/skinny_bf16_ab.py --out profiles/skinny_bf16_ab.txt
    python tools/skinny_bf16_ab.py --split --out profiles/skinny_split_ab.txt"""
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
SHAPES = [(1024, 1024), (4096, 4096), (4096, 1024), (1024, 4096), (1000, 1000)]
ROWS = [(2, m, n, K) for n, K in SHAPES for m in (1, 8, 16, 31)] + [(0, 8, 4096, 4096), (4, 8, 4096, 4096)]
INAME = {0: "flat", 2: "VNNI-2", 4: "VNNI-4"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--controls", action="store_true")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    pkg = importlib.import_module("tpp-mlir_amd")
    rt = pkg.get_runtime()
    has_switch = hasattr(rt, "set_skinny_bf16")
    has_split = hasattr(rt, "set_skinny_split")
    if args.split and not args.controls and not has_split:
        sys.exit("--split: this library has no xsmm_hip_set_skinny_split")
    torch.cuda.set_device(0)
    rt.set_async(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def mode(v, parts=0):
        if has_switch:
            rt.set_skinny_bf16(v)
        if has_split:
            rt.set_skinny_split(parts)

    def timed(run):
        run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    def rounds(sides, one):
        """one(side) -> us; warm-up of every side, then --pairs alternating rounds"""
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:
            for s in sides:
                one(s)
        t = {s: [] for s in sides}
        for _ in range(args.pairs):
            for s in sides:
                t[s].append(one(s))
        return t

    props = torch.cuda.get_device_properties(0)
    try:
        commit = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    if args.split:
        say("# K split across workgroups of the skinny-batch bf16 kernel (xsmm_hip_set_skinny_split): %s, one process, one GPU" % (
            "controls" if args.controls else "BN unsplit / BN with P = 2, 4, 8, 16 / mode 1 of both switches"))
    else:
        say("# skinny-batch bf16 layers (xsmm_hip_set_skinny_bf16): %s, one process, one GPU" % ("controls" if args.controls else "off / 16 / 32 / 64"))
    say("# box: %s, %d CUs; commit of the library's tree: %s, %s the switch; command: %s" % (
        props.name, props.multi_processor_count, commit, ("with" if has_split else "WITHOUT") if args.split else ("with" if has_switch else "WITHOUT"), " ".join(sys.argv)))
    say("# per side: %d invokes between two events, %d alternating rounds; us per invoke: median [min .. max]; B bytes / median" % (args.iters, args.pairs))
    say("# context: a device copy 6.29 TB/s, the Infinity Cache 8.6 TB/s (MI355X_MICROARCH)")

    if args.controls:
        sides = ["off"] + (["on"] if has_switch else [])
        # the 4096-row chain: three 1024-wide layers as one step of ShardedMlp
        spec = pkg.MlpSpec()
        x = (torch.rand(spec.batch, spec.layers[0], device="cuda") * 2 - 1).to(torch.bfloat16)
        ws = [(torch.rand(k * n, device="cuda") - 0.5).to(torch.bfloat16) for k, n in zip(spec.layers[:-1], spec.layers[1:])]
        bs = [(torch.rand(n, device="cuda") * 2 - 1).to(torch.bfloat16) for n in spec.layers[1:]]
        acts = [torch.zeros(spec.batch, n, device="cuda", dtype=torch.bfloat16) for n in spec.layers[1:]]
        mlp = pkg.ShardedMlp(spec, rt=rt)

        def chain(s):
            mode(1 if s == "on" else 0, 1 if s == "on" and args.split else 0)
            us = timed(lambda: mlp.forward(x, ws, bs, acts))
            mode(0)
            return us

        m = n = K = 1024
        A = (torch.rand(m, K, device="cuda") * 2 - 1).to(torch.bfloat16)
        B = (torch.rand(K * n, device="cuda") - 0.5).to(torch.bfloat16)
        C = torch.zeros(m, n, device="cuda", dtype=torch.bfloat16)
        D = (torch.rand(n, device="cuda") * 2 - 1).to(torch.bfloat16)
        h = rt.fused_brgemm_dispatch(BF16, m, n, 64, K, n, n, 64, 64 * n, 4 | VB, 0, 5, 4, 1)

        def call(s):
            mode(1 if s == "on" else 0, 1 if s == "on" and args.split else 0)
            us = timed(lambda: rt.fused_brgemm(BF16, h, A, 0, B, 0, C, 0, D, 0, K // 64))
            mode(0)
            return us

        for name, one in (("chain 4096 rows x [1024, 1024, 1024, 1024], one step (fused: %s)", chain), ("call 1024 x 1024 x 1024 VNNI-2%s", call)):
            t = rounds(sides, one)
            say(name % (mlp.last_step_fused if one is chain else ""))
            for s in sides:
                say("    %-3s %8.2f [%8.2f .. %8.2f]" % (s, statistics.median(t[s]), min(t[s]), max(t[s])))
    if not args.controls or args.split:
        for image, m, n, K in ROWS:
            k, br = (64, K // 64) if K % 64 == 0 else (K, 1)
            A = (torch.rand(m, K, device="cuda") * 2 - 1).to(torch.bfloat16)
            B = (torch.rand(K * n, device="cuda") - 0.5).to(torch.bfloat16)  # uniform data: the same buffer serves every image
            C = torch.zeros(m, n, device="cuda", dtype=torch.bfloat16)
            D = (torch.rand(n, device="cuda") * 2 - 1).to(torch.bfloat16)
            old = rt.set_vnni_factor(image) if image else None
            h = rt.fused_brgemm_dispatch(BF16, m, n, k, K, n, n, k, k * n, 4 | (VB if image else 0), 0, 5, 4, 1)
            if image:
                rt.set_vnni_factor(old)
            names = {}

            def one(s):
                if s == "rule":
                    mode(1, 1)
                else:
                    bn, _, parts = s.partition("/")
                    mode(0 if bn == "off" else int(bn), int(parts or 0))
                us = timed(lambda: rt.fused_brgemm(BF16, h, A, 0, B, 0, C, 0, D, 0, br))
                names[s] = rt.last_refined_kernel() or rt.kernel_name(h)
                mode(0)
                return us

            bns = [str(bn) for bn in (16, 32, 64) if not (image == 0 and bn == 16)]
            if args.controls:
                sides = ["off"]
            elif args.split:
                sides = [b + p for b in bns for p in ("", "/2", "/4", "/8", "/16")] + ["rule"]
            else:
                sides = ["off"] + (bns if has_switch else [])
            rule = "-"
            if has_switch:
                mode(1, 1 if args.split else 0)
                before, sbefore = rt.skinny_bf16_stats()[0], rt.skinny_split_stats()[0] if has_split else 0
                rt.fused_brgemm(BF16, h, A, 0, B, 0, C, 0, D, 0, br)
                torch.cuda.synchronize()
                after = rt.skinny_bf16_stats()
                rule = "BN %d" % after[3] if after[0] > before else "refuses"
                if has_split and args.split and after[0] > before:
                    rule += ", P %d" % rt.skinny_split_stats()[1] if rt.skinny_split_stats()[0] > sbefore else ", unsplit"
                mode(0)
            t = rounds(sides, one)
            med = {s: statistics.median(t[s]) for s in sides}
            say("%-6s m %2d  n %4d  K %4d (br %2d x k %4d)  B %5.2f MiB  mode 1: %s" % (INAME[image], m, n, K, br, k, 2.0 * K * n / 2 ** 20, rule))
            for s in sides:
                base = s.partition("/")[0] if args.split else "off"  # --split: the unsplit skinny side of the same BN
                wins = "" if s == base or base not in t else "  %+6.1f %%, faster than %s in %d of %d rounds" % (
                    100.0 * (med[s] - med[base]) / med[base], base, sum(b < a for a, b in zip(t[base], t[s])), args.pairs)
                say("    %-5s %8.2f [%8.2f .. %8.2f]  %5.2f TB/s  %s%s" % (s, med[s], min(t[s]), max(t[s]), 2.0 * K * n / med[s] * 1e-6, names[s], wins))
            if args.split and not args.controls:
                best = min(sides, key=lambda s_: med[s_])
                say("    best: %s %.2f us, %.2f TB/s (a device copy: 6.29 TB/s)" % (best, med[best], 2.0 * K * n / med[best] * 1e-6))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
