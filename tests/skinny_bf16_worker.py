"""Worker of tests/test_skinny_bf16_gpu.py, and the helpers the test shares with it. As a program (its own process: the mode and strict mode
come from the environment, read when the library is loaded): one skinny whole-layer bf16 call under TPP_HIP_SKINNY_BF16=<mode>, three times
on the same data. Prints one JSON line: the settings as the library read them, the kernel each call reported, the counters and a digest of
each result's bits.
  skinny_bf16_worker.py <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <k> <br> <seed>"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("tpp-mlir_amd")
from dma256_edge_worker import corner, embedded  # noqa: E402,F401
from dma256_images_worker import BF16, Case, digest  # noqa: E402,F401

KIND = {2: 0, 0: 2, 4: 4}  # Case.image -> what xsmm_hip_skinny_bf16_stats reports
SUFFIX = {2: "", 0: "_flatb", 4: "_vnni4"}
WMAX = 8  # SKN_WMAX of tpp-mlir_amd/csrc/brgemm_bf16_skinny.h


def instance_exists(image, bn):
    return bn in (16, 32, 64) and not (image == 0 and bn == 16)


def text(image, m, bn):
    return "brgemm_bf16_skinny%s<%dx%d>" % (SUFFIX[image], 16 if m <= 16 else 32, bn)


def expected_stats(count, image, n, k, br, bn):
    """xsmm_hip_skinny_bf16_stats after launch number `count`: workgroups, waves per workgroup, BN, B image - from the shape"""
    return (count, -(-n // bn), min(WMAX, br * -(-k // 32)), bn, KIND[image])


if __name__ == "__main__":
    image, m, n, k, br, seed = (int(x) for x in sys.argv[1:7])
    rt = pkg.get_runtime()
    mode = rt.set_skinny_bf16(0)  # what the library read from the environment
    rt.set_skinny_bf16(mode)
    out = {"from_env": mode, "strict": rt.get_strict(), "kernels": [], "digests": []}
    case = Case(image, m, n, k, br, seed)
    for _ in range(3):
        got, refined, _ = case.run(rt)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.skinny_bf16_stats())
    print(json.dumps(out))
