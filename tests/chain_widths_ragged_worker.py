"""Helper of tests/test_chain_widths_ragged_gpu.py and tests/test_chain_widths_ragged_exact_inputs.py, and the GPU test's worker. specs(t) is
the list of ragged mixed-width chains of tile t both files use (the GPU file runs them, the CPU file checks that their exact-input vectors
meet check_exact's precondition). As a program (its own process: strict mode is chosen before anything is queued; the switches and the
forced tile come from the environment): one ragged mixed-width bf16 chain under TPP_HIP_STRICT=1, TPP_HIP_CHAIN_WIDTHS_RAGGED=1 and
TPP_HIP_EDGE_TILES / _EDGE_K_BF16 / _EDGE_K8_BF16=<20 + t> through xsmm_hip_fused_brgemm_chain_invoke. Prints one JSON line: the settings as
the library read them, whether the chain ran as one launch, the counter and a digest of every layer's bits.
  chain_widths_ragged_worker.py <t> <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <seed> <n0,n1,..> <k0,k1,..>"""
import json
import sys

from chain_edge_worker import BF16, TILE, digest, pkg
from chain_widths_worker import WidthsChain

K0 = [72, 80, 88, 96, 104, 112, 120, 200]  # layer 0 of the "ragged k only" chain: every skip count 7 .. 1, and 200 (three whole chunks + 8)


def rows(t):
    bm = TILE[t][0]
    return [bm + 8, 3 * bm - 3]


def specs(t, mi):
    """(name, m, ns, ks, brs) of tile t's chains with m = rows(t)[mi]"""
    bm, bn = TILE[t]
    m = rows(t)[mi]
    chain = lambda ns, k0: (ns, [k0] + ns[:-1], [1] * len(ns))
    out = [("sit out and resume",) + (m,) + chain([3 * bn + 8, bn + 8, 2 * bn + 24], 192),
           ("first active layer > 0",) + (m,) + chain([bn + 8, 3 * bn, bn + 16], 128)]
    out += [("ragged k only, k0 = %d" % k0,) + (m,) + chain([4 * bn, 2 * bn, bn], k0) for k0 in K0]
    if mi == 1:
        out += [("ragged m only", 3 * bm - 3) + chain([3 * bn, bn, 2 * bn], 192)]
    out += [("twelve chunks", m, [2 * bn, bn], [200, 2 * bn], [3, 1]),
            ("eight layers",) + (m,) + chain([2 * bn + 8, bn + 8] * 4, 136),
            ("two batch elements", m, [2 * bn + 16, 2 * bn + 16, bn + 8], [144, bn + 8, bn + 8], [2, 2, 2])]
    return out


def launch_tile(t, image):
    """the tile a chain forced to tile t runs on: t, but for the one instance the mode does not have (64x128, VNNI-2) - there the smallest
    tile, which fits every shape of these files"""
    return 0 if (t == 2 and image == 2) else t


if __name__ == "__main__":
    t, image, m, seed = (int(x) for x in sys.argv[1:5])
    ns, ks = [int(x) for x in sys.argv[5].split(",")], [int(x) for x in sys.argv[6].split(",")]
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    out = {"strict": rt.get_strict(), "chain_widths_ragged_from_env": rt.set_chain_widths_ragged(1), "edge_tiles_from_env": rt.set_edge_tiles(20 + t)}
    ch = WidthsChain(rt, image, m, ns, ks, [1] * len(ns), seed)
    outs = ch.outputs()
    out["ran_as_one"] = bool(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
    got = ch.host(outs)
    ch.check_windows(got)
    out["digests"] = [digest(g) for g in got]
    out["chain_widths_ragged_stats"] = list(rt.chain_widths_ragged_stats())
    rt.set_chain_widths_ragged(0), rt.set_edge_tiles(0), rt.set_edge_k_bf16(0), rt.set_edge_k8_bf16(0), rt.set_async(was_async)
    print(json.dumps(out))
