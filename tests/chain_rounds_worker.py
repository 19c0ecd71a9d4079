"""Worker of tests/test_chain_rounds_gpu.py, and the shapes the test shares with it. As a program (its own process: strict mode is chosen
before anything is queued; it comes from the environment): one bf16 layer chain on tile t, the tile forced at dispatch, under
TPP_HIP_STRICT=1 - first the calls one by one with the switch off, then through xsmm_hip_fused_brgemm_chain_invoke under
TPP_HIP_CHAIN_ROUNDS=<1000 + G> as the library read it from the environment. Prints one JSON line: the settings as the library read them,
whether the chain ran as one launch, the counters and a digest of every layer's bits both ways.
  chain_rounds_worker.py <t> <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <shape index> <seed>"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("tpp-mlir_amd")
from chain_edge_worker import BASE, BF16, TILE, RaggedChain, digest  # noqa: E402

NSLOT = [8, 8, 6, 4]  # ring slots of tile t's chain instance: a layer of 64 * NSLOT k makes the B loaders run ahead


def shapes(t):
    """(m, n, k per layer, batch elements per layer, G) on tile t: uneven groups (3 and 2 row blocks), even groups, one group that walks
    every block, layers of exactly NSLOT chunks (the B loaders run ahead across steps), two batch elements per layer with stride_a along k"""
    bm, bn = TILE[t]
    ns = 64 * NSLOT[t]
    return [(5 * bm, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 2),
            (4 * bm, bn, [192, bn, bn], [1, 1, 1], 2),
            (3 * bm, 2 * bn, [192, 2 * bn, 2 * bn], [1, 1, 1], 1),
            (3 * bm, ns, [ns, ns, ns], [1, 1, 1], 2),
            (5 * bm, 2 * bn, [128, bn, bn], [2, 2, 2], 2)]


def make(rt, t, image, shape, seed, exact=False, **kw):
    m, n, ks, brs, _ = shape
    return RaggedChain(rt, image, m, n, ks, brs, seed, exact=exact, force=BASE[image] + t, **kw)


if __name__ == "__main__":
    t, image, index, seed = (int(x) for x in sys.argv[1:5])
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    shape = shapes(t)[index]
    mode = rt.set_chain_rounds(0)  # (what the library read from the environment)
    out = {"strict": rt.get_strict(), "chain_rounds_from_env": mode}
    ch = make(rt, t, image, shape, seed)
    outs = ch.outputs()
    ch.one_by_one(outs)
    got = ch.host(outs)
    ch.check_windows(got)
    out["separate"] = [digest(g) for g in got]
    rt.set_chain_rounds(mode)
    outs = ch.outputs()
    out["ran_as_one"] = bool(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
    got = ch.host(outs)
    ch.check_windows(got)
    out["digests"] = [digest(g) for g in got]
    out["chain_rounds_stats"] = list(rt.chain_rounds_stats())
    out["chain_edge_launches"] = rt.chain_edge_stats()[0]
    out["edge_tiles_launches"] = rt.edge_tiles_stats()[0]
    rt.set_chain_rounds(0), rt.set_async(was_async)
    print(json.dumps(out))
