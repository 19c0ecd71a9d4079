"""Helper of tests/test_chain_width_rounds_gpu.py, and its worker. The chains are chain_widths_worker.WidthsChain's. As a program (its own
process: strict mode is chosen before anything is queued; the switch comes from the environment): one mixed-width chain whose calls are
dispatched on DIFFERENT tiles, under TPP_HIP_STRICT=1 and TPP_HIP_CHAIN_WIDTH_ROUNDS=1 through xsmm_hip_fused_brgemm_chain_invoke. Prints one
JSON line: the settings as the library read them, whether the chain ran as one launch, the counters and a digest of every layer's bits.
  chain_width_rounds_worker.py <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <seed> <n0,n1,..> <tile of call 0,tile of call 1,..>"""
import json
import sys

from chain_edge_worker import BF16, digest, pkg
from chain_widths_worker import WidthsChain


def balanced_w(max_t, tiles_m, cus):
    """brgemm_bf16_lw_chain_wrounds.h chain_wrounds_max_groups / chain_wrounds_groups: the rule's W (0: none fits)"""
    wfit = min(max_t - 1, cus // tiles_m)
    if wfit < 1:
        return 0
    rounds = -(-max_t // wfit)
    return -(-max_t // rounds)


if __name__ == "__main__":
    image, m, seed = (int(x) for x in sys.argv[1:4])
    ns, tiles = [int(x) for x in sys.argv[4].split(",")], [int(x) for x in sys.argv[5].split(",")]
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    out = {"strict": rt.get_strict(), "chain_width_rounds_from_env": rt.set_chain_width_rounds(1)}
    try:
        ch = WidthsChain(rt, image, m, ns, [192] + ns[:-1], [1] * len(ns), seed, tiles=tiles)
        outs = ch.outputs()
        out["ran_as_one"] = bool(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
        got = ch.host(outs)
        ch.check_windows(got)
        out["digests"] = [digest(g) for g in got]
        out["chain_width_rounds_stats"] = list(rt.chain_width_rounds_stats())
        out["chain_widths_stats"] = list(rt.chain_widths_stats())
    finally:
        rt.set_chain_width_rounds(0), rt.set_async(was_async)
    print(json.dumps(out))
