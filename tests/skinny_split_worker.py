"""Worker of tests/test_skinny_split_gpu.py, and the helpers the test shares with it. As a program (its own process: both modes and strict
mode come from the environment, read when the library is loaded): one skinny whole-layer bf16 call under TPP_HIP_SKINNY_BF16=<BN> and
TPP_HIP_SKINNY_SPLIT=<P>, three times on the same data. Prints one JSON line: the settings as the library read them, the kernel each call
reported, both counters and a digest of each result's bits.
  skinny_split_worker.py <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <k> <br> <seed>"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("tpp-mlir_amd")
from skinny_bf16_worker import KIND, SUFFIX, WMAX, Case, digest  # noqa: E402,F401


def steps(k, br):
    return br * -(-k // 32)


def parts(P, k, br):
    """P_eff: a part has at least one 32-k step"""
    return min(P, steps(k, br))


def text(image, m, bn):
    return "brgemm_bf16_skinny_split%s<%dx%d>" % (SUFFIX[image], 16 if m <= 16 else 32, bn)


def expected_split_stats(count, n, k, br, bn, P):
    """xsmm_hip_skinny_split_stats after split launch number `count`: P_eff, workgroups"""
    return (count, parts(P, k, br), -(-n // bn) * parts(P, k, br))


def expected_skinny_stats(count, image, n, k, br, bn, P):
    """xsmm_hip_skinny_bf16_stats after a split launch: workgroups = column blocks * P_eff, the waves of part 0 (the longest run), BN, image"""
    pe = parts(P, k, br)
    return (count, -(-n // bn) * pe, min(WMAX, -(-steps(k, br) // pe)), bn, KIND[image])


if __name__ == "__main__":
    image, m, n, k, br, seed = (int(x) for x in sys.argv[1:7])
    rt = pkg.get_runtime()
    bn, P = rt.set_skinny_bf16(0), rt.set_skinny_split(0)  # what the library read from the environment
    rt.set_skinny_bf16(bn)
    rt.set_skinny_split(P)
    out = {"from_env": [bn, P], "strict": rt.get_strict(), "kernels": [], "digests": []}
    case = Case(image, m, n, k, br, seed)
    for _ in range(3):
        got, refined, _ = case.run(rt)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.skinny_bf16_stats())
    out["split_stats"] = list(rt.skinny_split_stats())
    print(json.dumps(out))
