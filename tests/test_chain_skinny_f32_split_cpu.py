"""The K split inside a skinny-batch f32 chain launch (include/tpp_xsmm_abi.h xsmm_hip_set_chain_skinny_f32_split) without a GPU: the schedule of
brgemm_f32_skinny_chain_split.h walked as the kernel walks it, plan_chain's answers with the real gemm_plan.cpp at 256 CUs
(tests/chain_skinny_f32_split/driver.cpp, a stand-alone program), and the switch's plumbing."""
import importlib
import os
import re
import subprocess
import sys

import pytest

from test_chain_skinny_f32_cpu import F32_BRANCH, PLAN, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
pkg = importlib.import_module("tpp-mlir_amd")
PS = [2, 3, 16]


def chains(bn):
    """the two chains of tests/test_chain_skinny_f32_split_gpu.py: (id, n per layer, k per layer, batch per layer).
    a: k0 = 36 is 3 steps - P 16 becomes P_l 3, P 2 deals 2 + 1 -, the last block of layer 0 is shifted back.
    b: a layer of one block (most workgroups sit it out or hold parts only; one step at BN 16: P_l 1), a wide ragged one, a batch of 2."""
    return [("a", [3 * bn + 4, 2 * bn], [36, 3 * bn + 4], [1, 1]),
            ("b", [bn, 7 * bn - 4, bn + 8], [32, bn, 7 * bn - 4], [2, 1, 1])]


def schedule(bn, mb, P, ns, ks, brs):
    """per layer (column blocks, steps, P_l); units of the widest layer, waves, scratch floats and counters of the launch"""
    layers = [(-(-n // bn), br * -(-k // 16), min(P, br * -(-k // 16))) for n, k, br in zip(ns, ks, brs)]
    return (layers, max(b * p for b, _, p in layers), max(min(8, -(-s // p)) for _, s, p in layers),
            max(b * p * mb * bn if p >= 2 else 0 for b, _, p in layers), max(b if p >= 2 else 0 for b, _, p in layers))


def csv(x):
    return ",".join(str(v) for v in x)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain_skinny_f32_split")
    objs = []
    for src in (os.path.join(CSRC, "gemm_plan.cpp"), os.path.join(ROOT, "tests", "chain_skinny_f32_split", "driver.cpp")):
        objs.append(str(d / (os.path.basename(src) + ".o")))
        subprocess.check_call([build.hipcc()] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", objs[-1]])
    subprocess.check_call([build.hipcc(), "--offload-arch=" + build.ARCH] + objs + ["-o", str(d / "driver")])
    return lambda *a: subprocess.run([str(d / "driver")] + [str(x) for x in a], capture_output=True, text=True, check=True, timeout=300).stdout


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("bn", [16, 32, 64])
def test_every_unit_owned_once_parts_cover_the_steps_every_workgroup_arrives_once_the_scratch_holds(driver, bn, P):
    for name, ns, ks, brs in chains(bn):
        for m in (16, 17):
            layers, units, waves, floats, counters = schedule(bn, 16 if m <= 16 else 32, P, ns, ks, brs)
            total = sum(b * p for b, _, p in layers)
            for G in sorted({1, 3, units, units + 5}):
                want = "once %d of %d arrivals %d..%d waves %d floats %d counters %d bad 0\n" % (total, total, G, G, waves, floats, counters)
                assert driver("walk", bn, m, G, P, csv(ns), csv(ks), csv(brs)) == want, (name, m, G)


N, K, FUNNEL = [72, 64], [64, 72], ([512, 256, 128], [784, 512, 256])
# (mode, split, strict, m, n per layer, k per layer) -> the row of tests/test_chain_skinny_f32_cpu.py PLAN it must still answer with the split at 0
# and at 1 (mode 1 of the split takes none of these rows: profiles/chain_skinny_f32_split_ab.txt)
UNCHANGED = [((16, N, K), "forced 16"), ((32, N, K), "forced 32"), ((64, N, K), "forced 64"), ((1, *FUNNEL), "mode 1, funnel m 16"), ((0, N, K), "switch 0, m 16")]


def test_plan_chain_split_off_answers_as_before_forced_parts_are_clipped_by_the_steps(driver):
    def plan(mode, split, strict, m, ns, ks, brs=None):
        return driver("plan", mode, split, int(strict), m, csv(ns), csv(ks), csv(brs or [1] * len(ns))).strip()
    for (mode, ns, ks), row in UNCHANGED:
        for split in (0, 1) + ((4,) if mode == 0 else ()):  # (mode 0: the switch alone changes nothing)
            got = plan(mode, split, False, 16, ns, ks)
            assert got == PLAN[row] + ("" if PLAN[row] == F32_BRANCH else " parts 0 layer parts" + " 1" * len(ns)), (row, split)
    # forced P: 72 x 64 has 4 steps, 64 x 72 has 5; BN 16: 5 and 4 blocks -> units 20 / 20 at P 4, 20 / 20 at P 16 (P_l 4, 5)
    assert plan(16, 4, False, 16, N, K) == "form 11 tile 16 groups 20 key 1 20 pad 0 parts 4 layer parts 4 4"
    assert plan(16, 16, False, 16, N, K) == "form 11 tile 16 groups 20 key 1 20 pad 0 parts 16 layer parts 4 5"
    assert plan(2016, 3, False, 31, N, K) == "form 11 tile 16 groups 2 key 1 2 pad 0 parts 3 layer parts 3 3"  # a forced G stays
    assert plan(64, 2, False, 1, [4096, 4096], [4096, 4096]) == "form 11 tile 64 groups 128 key 1 128 pad 0 parts 2 layer parts 2 2"
    assert plan(16, 16, False, 1, [4096, 4096], [4096, 4096]).startswith("form 11 tile 16 groups 256 key 1 256 pad 0 parts 16")  # G <= CUs
    assert plan(16, 2, False, 16, [16, 16], [16, 16]).endswith("parts 0 layer parts 1 1"), "no layer has two steps: the unsplit launch"
    # mode 1 of the split, as fitted to profiles/chain_skinny_f32_split_ab.txt: 4096-wide at m 31 on BN 32 with P 2, under mode 1 and under a forced BN 32
    wide = ([4096] * 3, [4096] * 3)
    assert plan(1, 1, False, 31, *wide) == plan(32, 1, False, 31, *wide) == "form 11 tile 32 groups 256 key 1 256 pad 0 parts 2 layer parts 2 2 2"
    assert plan(1, 1, False, 16, *wide) == plan(1, 0, False, 31, *wide) == F32_BRANCH and plan(16, 1, False, 31, *wide).endswith("parts 0 layer parts 1 1 1")
    assert plan(1, 4, False, 17, *FUNNEL) == F32_BRANCH, "a forced P does not lift mode 1's gate"
    assert plan(32, 4, True, 16, N, K) == F32_BRANCH, "strict mode refuses"
    assert plan(300032, 4, False, 16, N, K) == F32_BRANCH, "a forced G above the CUs refuses"


def test_setter_environment_and_counter_plumbing():
    pkg.build()
    rt = pkg.get_runtime()
    prev, last = rt.set_chain_skinny_f32_split(0), 0
    for v in list(range(17)) + [-1, 17, 1016, prev]:
        ok = 0 <= v <= 16
        assert rt.set_chain_skinny_f32_split(v) == (last if ok else -1), v
        last = v if ok else last
    assert len(rt.chain_skinny_f32_split_stats()) == 3
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        assert re.findall(r"TPP_XSMM_EXPORT\s+void\s+xsmm_hip_chain_skinny_f32_split_stats\s*\(\s*int64_t\s+out\[(\d+)\]", f.read()) == ["3"]
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(list(rt.chain_skinny_f32_split_stats()), rt.set_chain_skinny_f32_split(0), rt.set_chain_skinny_f32(0), rt.set_skinny_f32_split(0))" % ROOT)
    for text, want in (("4", 4), ("17", 0), ("-1", 0)):
        env = dict({k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}, TPP_HIP_CHAIN_SKINNY_F32_SPLIT=text)
        assert subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1] == "[0, 0, 0] %d 0 0" % want
