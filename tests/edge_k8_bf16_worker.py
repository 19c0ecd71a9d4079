"""Worker of tests/test_edge_k8_bf16_gpu.py. As a program (its own process: strict mode is chosen before anything is queued, the half-step
ragged-k mode comes from the environment): one whole-layer bf16 call with a ragged k under TPP_HIP_STRICT=1 and
TPP_HIP_EDGE_K8_BF16=<mode>, three times on the same data. Prints one JSON line: the settings as the library read them, the kernel each
call reported, the counters and a digest of each result's bits. The call helpers are those of tests/edge_k_bf16_worker.py.
  edge_k8_bf16_worker.py <mode> <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <k> <br> <seed>"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("tpp-mlir_amd")
from edge_k_bf16_worker import digest, layer_call, operands  # noqa: E402

if __name__ == "__main__":
    mode, image, m, n, k, br, seed = (int(x) for x in sys.argv[1:8])
    rt = pkg.get_runtime()
    out = {"strict": rt.get_strict(), "edge_k8_bf16_from_env": rt.set_edge_k8_bf16(mode), "kernels": [], "digests": []}
    A, B, C, D = operands(m, n, k, br, seed)
    for _ in range(3):
        got, refined = layer_call(rt, image, m, n, k, br, A, B, C, D)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.edge_k8_bf16_stats())
    out["older_stats"] = [list(rt.edge_k_bf16_stats()), list(rt.edge_k_stats()), list(rt.edge_tiles_stats())]
    print(json.dumps(out))
