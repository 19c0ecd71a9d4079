"""Worker of tests/test_dma256_edge_gpu.py, and the helpers the test shares with it. As a program (its own process: the mode and strict
mode come from the environment, read when the library is loaded): one ragged whole-layer bf16 call under TPP_HIP_DMA256_EDGE=<mode>, three
times on the same data. Prints one JSON line: the settings as the library read them, the kernel each call reported, the counters and a
digest of each result's bits.
  dma256_edge_worker.py <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <k> <br> <seed>"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("tpp-mlir_amd")
from dma256_images_worker import BF16, Case, digest  # noqa: E402,F401


def up256(x):
    return -(-x // 256) * 256


def embedded(big, m, n, seed):
    """the m x n corner of the call `big` (a Case of M x N, M >= m, N >= n) as a call of its own, in buffers of its own layout: the first m
    rows of A, the first n columns of B, of the bias row and of C hold big's values - everything else is what a Case of m x n holds there
    (NaN in gaps and guards, a bit pattern around C)"""
    c = Case(big.image, m, n, big.k, big.br, seed, beta0=big.beta0, bias=big.bias, relu=big.relu)
    ii, kk, jj = np.arange(m)[:, None], np.arange(big.k)[None, :], np.arange(n)[None, :]
    for b in range(max(big.br, 1)):
        c.A[(c.offs[0] + b * c.sa + ii * c.lda + kk).reshape(-1)] = big.A[(big.offs[0] + b * big.sa + ii * big.lda + kk).reshape(-1)]
        kr = np.arange(big.k)[:, None]
        c.B[c.b_index(b, kr, jj).reshape(-1)] = big.B[big.b_index(b, kr, jj).reshape(-1)]
    c.D[c.offs[3]:c.offs[3] + n] = big.D[big.offs[3]:big.offs[3] + n]
    if not big.beta0:
        c.C[c.win] = big.C[(big.offs[2] + ii * big.ldc + jj).reshape(-1)]
    return c


def corner(big, got, m, n):
    """the m x n corner of big's C buffer `got`"""
    ii, jj = np.arange(m)[:, None], np.arange(n)[None, :]
    return got[(big.offs[2] + ii * big.ldc + jj).reshape(-1)]


if __name__ == "__main__":
    image, m, n, k, br, seed = (int(x) for x in sys.argv[1:7])
    rt = pkg.get_runtime()
    mode = rt.set_dma256_edge(0)  # what the library read from the environment
    rt.set_dma256_edge(mode)
    out = {"from_env": mode, "strict": rt.get_strict(), "kernels": [], "digests": []}
    case = Case(image, m, n, k, br, seed)
    for _ in range(3):
        got, refined, _ = case.run(rt)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.dma256_edge_stats())
    print(json.dumps(out))
