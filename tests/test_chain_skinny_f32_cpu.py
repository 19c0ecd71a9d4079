"""Skinny-batch f32 layer chains (include/tpp_xsmm_abi.h xsmm_hip_set_chain_skinny_f32) without a GPU: the schedule of
brgemm_f32_skinny_chain.h walked as the kernel walks it, plan_chain's answers with the real gemm_plan.cpp at 256 CUs
(tests/chain_skinny_f32/driver.cpp, a stand-alone program), and the switch's plumbing."""
import importlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
pkg = importlib.import_module("tpp-mlir_amd")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402


def chains(bn):
    """the chains of tests/test_chain_skinny_f32_gpu.py: (id, n per layer, k per layer, batch per layer)"""
    return [("ragged_k", [3 * bn + 4] * 3, [36, 3 * bn + 4, 3 * bn + 4], [1, 1, 1]),
            ("sit_out", [4 * bn, bn, 2 * bn + 4], [32, 4 * bn, bn], [1, 1, 1]),
            ("waves_1_8", [132, max(36, bn), bn], [16, 132, 16], [1, 1, 1]),  # (36 columns are no block of BN 64: the launch needs n_l >= BN)
            ("batches", [144, 96, 64], [20, 36, 16], [2, 2, 3]),
            ("eight_layers", [2 * bn + 4, bn + 4] * 4, [32] + [2 * bn + 4, bn + 4] * 3 + [2 * bn + 4], [1] * 8),
            ("forced_G", [6 * bn + 4] * 2, [36, 6 * bn + 4], [1, 1])]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain_skinny_f32")
    objs = []
    for src in (os.path.join(CSRC, "gemm_plan.cpp"), os.path.join(ROOT, "tests", "chain_skinny_f32", "driver.cpp")):
        objs.append(str(d / (os.path.basename(src) + ".o")))
        subprocess.check_call([build.hipcc()] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", objs[-1]])
    subprocess.check_call([build.hipcc(), "--offload-arch=" + build.ARCH] + objs + ["-o", str(d / "driver")])
    return lambda *a: subprocess.run([str(d / "driver")] + [str(x) for x in a], capture_output=True, text=True, check=True, timeout=300).stdout


@pytest.mark.parametrize("bn", [16, 32, 64])
def test_every_block_owned_once_every_workgroup_arrives_once_the_waves_are_the_single_call_s(driver, bn):
    for name, ns, ks, brs in chains(bn):
        blocks = [-(-n // bn) for n in ns]
        waves = max(min(8, br * -(-k // 16)) for k, br in zip(ks, brs))
        for G in sorted({max(blocks), 1, 3, 7}):
            want = "once %d of %d arrivals %d..%d waves %d bad 0\n" % (sum(blocks), sum(blocks), G, G, waves)
            assert driver("walk", bn, G, *(",".join(str(v) for v in x) for x in (ns, ks, brs))) == want, (name, G)


F32_BRANCH = "calls : an f32 call is not beta 0 / not planned on the K-split loader-wave tile of the first call"
# form 11 = CF_SKINNY_F32 behind CF_SKINNY = 10; key (1, G); "switch 0" and m >= 32: the parent's answers (form 1 = CF_F32 on its tile 2, 8 x 32 tiles)
PLAN = {"forced 16": "form 11 tile 16 groups 5 key 1 5 pad 0", "forced 32": "form 11 tile 32 groups 3 key 1 3 pad 0", "forced 64": "form 11 tile 64 groups 2 key 1 2 pad 0",
        "forced G 2 BN 32": "form 11 tile 32 groups 2 key 1 2 pad 0", "three layers 16": "form 11 tile 16 groups 9 key 1 9 pad 0",
        "strict": F32_BRANCH, "n % 4 != 0": F32_BRANCH, "k % 4 != 0": F32_BRANCH, "n_l < BN": F32_BRANCH, "m = 32": F32_BRANCH, "beta 1": F32_BRANCH,
        "forced G above the CUs": F32_BRANCH, "switch 0, m 16": F32_BRANCH,
        # mode 1 as fitted to profiles/chain_skinny_f32_ab.txt: BN 16 up to the funnel's largest layer at m <= 16, up to 4 MiB at m = 1
        "mode 1, funnel m 16": "form 11 tile 16 groups 32 key 1 32 pad 0", "mode 1, funnel m 17": F32_BRANCH,
        "mode 1, 1024 m 1": "form 11 tile 16 groups 64 key 1 64 pad 0", "mode 1, 1024 m 2": F32_BRANCH, "mode 1, 1028 m 1": F32_BRANCH,
        "switch 0, m 512": "form 1 tile 2 groups 0 key 8 32 pad 0", "forced 32, m 512": "form 1 tile 2 groups 0 key 8 32 pad 0"}


def test_plan_chain_takes_under_forced_modes_and_answers_as_before_otherwise(driver):
    got = dict(l.split(" : ", 1) for l in driver("plan").splitlines() if " : " in l)
    bf16 = got.pop("bf16")
    assert bf16.startswith("calls : ") and "f32" not in bf16, bf16
    assert got == PLAN
    assert driver("plan").splitlines()[-1] == "ld_ok 1 0 0 0 1 0 0"


def test_setter_environment_and_counter_plumbing():
    pkg.build()
    rt = pkg.get_runtime()
    prev, last = rt.set_chain_skinny_f32(0), 0
    for v in [0, 1, 16, 32, 64, 1016, 7064, 512032, 2, 48, 1000, 1017, 513016, -1, prev]:
        bn, g = (v % 1000, v // 1000) if v >= 1000 else (v, 1)
        ok = v in (0, 1) or (bn in (16, 32, 64) and 1 <= g <= 512)
        assert rt.set_chain_skinny_f32(v) == (last if ok else -1), v
        last = v if ok else last
    assert len(rt.chain_skinny_f32_stats()) == 4
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        assert re.findall(r"TPP_XSMM_EXPORT\s+void\s+xsmm_hip_chain_skinny_f32_stats\s*\(\s*int64_t\s+out\[(\d+)\]", f.read()) == ["4"]
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(list(rt.chain_skinny_f32_stats()), rt.set_chain_skinny_f32(0), rt.set_chain_skinny(0), rt.set_skinny_f32(0))" % ROOT)
    for text, want in (("3032", 3032), ("48", 0), ("-1", 0)):
        env = dict({k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}, TPP_HIP_CHAIN_SKINNY_F32=text)
        assert subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1] == "[0, 0, 0, 0] %d 0 0" % want
