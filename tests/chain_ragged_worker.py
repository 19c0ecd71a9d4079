"""Worker of tests/test_chain_ragged_gpu.py. A program (its own process: strict mode is chosen before anything is queued; the switches and the
forced tile come from the environment): one ragged-width bf16 layer chain under TPP_HIP_STRICT=1, TPP_HIP_CHAIN_RAGGED=1 and TPP_HIP_EDGE_TILES /
_EDGE_K_BF16 / _EDGE_K8_BF16=<20 + t> through xsmm_hip_fused_brgemm_chain_invoke. Prints one JSON line: the settings as the library read them,
whether the chain ran as one launch, the counter and a digest of every layer's bits.
  chain_ragged_worker.py <t> <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <seed>"""
import json
import sys

from chain_edge_worker import BF16, RaggedChain, digest, pkg

if __name__ == "__main__":
    t, image, m, n, seed = (int(x) for x in sys.argv[1:6])
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    out = {"strict": rt.get_strict(), "chain_ragged_from_env": rt.set_chain_ragged(1), "edge_tiles_from_env": rt.set_edge_tiles(20 + t)}
    ch = RaggedChain(rt, image, m, n, [200, n, n], [1, 1, 1], seed)
    outs = ch.outputs()
    out["ran_as_one"] = bool(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
    got = ch.host(outs)
    ch.check_windows(got)
    out["digests"] = [digest(g) for g in got]
    out["chain_ragged_stats"] = list(rt.chain_ragged_stats())
    rt.set_chain_ragged(0), rt.set_edge_tiles(0), rt.set_edge_k_bf16(0), rt.set_edge_k8_bf16(0), rt.set_async(was_async)
    print(json.dumps(out))
