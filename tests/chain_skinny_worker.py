"""Worker of tests/test_chain_skinny_gpu.py, and the helpers the test shares with it. As a program (its own process: strict mode is chosen
before anything is queued; the switch comes from the environment): one skinny-batch chain through xsmm_hip_fused_brgemm_chain_invoke with
the switch as the library read it, then with the switch 0. Prints one JSON line: the settings as the library read them, whether each run
was one launch, the counter and a digest of every layer's bits of both runs.
  chain_skinny_worker.py <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <seed> <n0,n1,..> <k0>"""
import json
import sys

from chain_edge_worker import BF16, digest, pkg
from chain_widths_worker import WidthsChain

KIND = {2: 0, 0: 2, 4: 4}  # WidthsChain's image (the VNNI factor, 0 flat) -> the B image as the library counts it
WMAX = 8                   # SKN_WMAX of tpp-mlir_amd/csrc/brgemm_bf16_skinny.h


def instance_exists(image, bn):
    return bn in (16, 32, 64) and not (image == 0 and bn == 16)


def blocks(n, bn):
    return -(-n // bn)


def groups(ns, bn, cus):
    """G of modes 1 / 16 / 32 / 64: a workgroup per column block of the widest layer, at most the compute units"""
    return min(max(blocks(n, bn) for n in ns), cus)


def run_chain(rt, ch, outs=None):
    """one chain invoke on fresh (or refilled) outputs: (ran as one launch, the layers on the host), windows checked"""
    if outs is None:
        outs = ch.outputs()
    else:
        ch.refill(outs)
    ran = bool(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
    got = ch.host(outs)
    ch.check_windows(got)
    return ran, got


if __name__ == "__main__":
    image, m, seed = (int(x) for x in sys.argv[1:4])
    ns, k0 = [int(x) for x in sys.argv[4].split(",")], int(sys.argv[5])
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    mode = rt.set_chain_skinny(0)
    rt.set_chain_skinny(mode)
    out = {"strict": rt.get_strict(), "chain_skinny_from_env": mode}
    ch = WidthsChain(rt, image, m, ns, [k0] + ns[:-1], [1] * len(ns), seed, exact=True)
    ran, got = run_chain(rt, ch)
    out["ran_as_one"], out["digests"] = ran, [digest(g) for g in got]
    out["chain_skinny_stats"] = list(rt.chain_skinny_stats())
    rt.set_chain_skinny(0)
    ran, got = run_chain(rt, ch)
    out["ran_as_one_off"], out["digests_off"] = ran, [digest(g) for g in got]
    rt.set_async(was_async)
    print(json.dumps(out))
