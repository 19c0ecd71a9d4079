"""The K split inside a skinny-batch bf16 chain launch (include/tpp_xsmm_abi.h xsmm_hip_set_chain_skinny_split) without a GPU: the schedule of
brgemm_bf16_skinny_chain_split.h walked as the kernel walks it, plan_chain_skinny's answers with the real gemm_plan.cpp at 256 CUs
(tests/chain_skinny_split/driver.cpp, a stand-alone program), and the switch's plumbing."""
import importlib
import os
import re
import subprocess
import sys

import pytest

from test_chain_skinny_gpu import chains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tpp-mlir_amd", "csrc")
pkg = importlib.import_module("tpp-mlir_amd")
sys.path.insert(0, os.path.join(ROOT, "tpp-mlir_amd"))
import build  # noqa: E402

PS = [2, 3, 16]


def schedule(bn, mb, P, ns, ks, brs):
    """per layer (column blocks, steps, P_l); units of the layer with the most, waves, scratch floats and counters of the launch"""
    layers = [(-(-n // bn), br * -(-k // 32), min(P, br * -(-k // 32))) for n, k, br in zip(ns, ks, brs)]
    return (layers, max(b * p for b, _, p in layers), max(min(8, -(-s // p)) for _, s, p in layers),
            max(b * p * mb * bn if p >= 2 else 0 for b, _, p in layers), max(b if p >= 2 else 0 for b, _, p in layers))


def csv(x):
    return ",".join(str(v) for v in x)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain_skinny_split")
    objs = []
    for src in (os.path.join(CSRC, "gemm_plan.cpp"), os.path.join(ROOT, "tests", "chain_skinny_split", "driver.cpp")):
        objs.append(str(d / (os.path.basename(src) + ".o")))
        subprocess.check_call([build.hipcc()] + build.FLAGS + ["-x", "hip", "-I" + CSRC, "-c", src, "-o", objs[-1]])
    subprocess.check_call([build.hipcc(), "--offload-arch=" + build.ARCH] + objs + ["-o", str(d / "driver")])
    return lambda *a: subprocess.run([str(d / "driver")] + [str(x) for x in a], capture_output=True, text=True, check=True, timeout=300).stdout


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("bn", [16, 32, 64])
def test_every_unit_owned_once_parts_cover_the_steps_every_workgroup_arrives_once_the_scratch_holds(driver, bn, P):
    """(the driver counts as bad: a unit off the walk, a part whose waves do not cover its run once and in order, a block without P_l parts,
    parts that do not cover the steps, a one-step layer with more than one part, a parked float or a counter beyond what the launch asks for)"""
    for name, ns, ks, brs in chains(bn):
        for m in (16, 17):
            layers, units, waves, floats, counters = schedule(bn, 16 if m <= 16 else 32, P, ns, ks, brs)
            total = sum(b * p for b, _, p in layers)
            for G in sorted({1, 3, units, units + 5}):
                want = "once %d of %d arrivals %d..%d waves %d floats %d counters %d bad 0\n" % (total, total, G, G, waves, floats, counters)
                assert driver("walk", bn, m, G, P, csv(ns), csv(ks), csv(brs)) == want, (name, m, G)


N, K = [72, 64], [64, 72]  # 2 and 3 steps


def test_plan_chain_skinny_split_off_answers_as_before_forced_parts_are_clipped_by_the_steps(driver):
    def plan(mode, split, strict, m, ns, ks, image=0, brs=None):
        return driver("plan", mode, split, int(strict), m, image, csv(ns), csv(ks), csv(brs or [1] * len(ns))).splitlines()
    wide = ([4096] * 3, [4096] * 3)
    for mode, strict, m, image, shape in ((16, False, 16, 0, (N, K)), (32, False, 31, 2, (N, K)), (2064, False, 1, 4, (N, K)), (1, False, 8, 0, ([1024] * 3, [1024] * 3)),
                                          (1, False, 8, 0, wide), (1, False, 8, 2, (N, K)), (0, False, 16, 0, (N, K)), (32, True, 16, 0, (N, K)), (300032, False, 16, 0, (N, K))):
        with_arg, without = plan(mode, 0, strict, m, *shape, image=image)
        assert with_arg == without and " parts 0 " in with_arg, (mode, m, image)
        if mode == 0:  # the switch alone changes nothing
            assert plan(0, 4, strict, m, *shape, image=image) == [without]
    # forced P: BN 16 has 5 and 4 blocks -> P 2: units 10 / 8; P 16: P_l 2 and 3, units 10 / 12
    assert plan(16, 2, False, 16, N, K) == ["bn 16 groups 10 gated 0 parts 2 why '' layer parts 2 2"]
    assert plan(16, 16, False, 16, N, K) == ["bn 16 groups 12 gated 0 parts 16 why '' layer parts 2 3"]
    assert plan(2016, 3, False, 31, N, K) == ["bn 16 groups 2 gated 0 parts 3 why '' layer parts 2 3"]  # a forced G stays
    assert plan(64, 2, False, 1, *wide) == ["bn 64 groups 128 gated 0 parts 2 why '' layer parts 2 2 2"]
    assert plan(16, 16, False, 1, *wide)[0].startswith("bn 16 groups 256 gated 0 parts 16 ")  # G <= CUs
    assert plan(16, 2, False, 16, [16, 16], [32, 16])[0].endswith("parts 0 why '' layer parts 1 1"), "no layer has two steps: the unsplit launch"
    # a forced P lifts no gate of mode 1; mode 1 of the split takes nothing beyond its measured rows
    for image, shape in ((0, wide), (2, (N, K))):
        gated = plan(1, 0, False, 8, *shape, image=image)[0]
        assert " gated 1 " in gated and " gated 1 " in plan(1, 4, False, 8, *shape, image=image)[0]
    assert plan(1, 1, False, 8, [1024] * 3, [1024] * 3) == [plan(1, 0, False, 8, [1024] * 3, [1024] * 3)[0]]
    assert plan(32, 4, True, 16, N, K)[0].startswith("bn 0 groups 0 gated 0 parts 0 why 'strict mode")
    assert plan(300032, 4, False, 16, N, K)[0].startswith("bn 0 groups 0 gated 0 parts 0 why 'more resident workgroups forced")


def test_setter_environment_and_counter_plumbing():
    pkg.build()
    rt = pkg.get_runtime()
    prev, last = rt.set_chain_skinny_split(0), 0
    for v in list(range(17)) + [-1, 17, 1016, prev]:
        ok = 0 <= v <= 16
        assert rt.set_chain_skinny_split(v) == (last if ok else -1), v
        last = v if ok else last
    assert len(rt.chain_skinny_split_stats()) == 3
    with open(os.path.join(ROOT, "include", "tpp_xsmm_abi.h")) as f:
        assert re.findall(r"TPP_XSMM_EXPORT\s+void\s+xsmm_hip_chain_skinny_split_stats\s*\(\s*int64_t\s+out\[(\d+)\]", f.read()) == ["3"]
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('tpp-mlir_amd').get_runtime(); "
            "print(list(rt.chain_skinny_split_stats()), rt.set_chain_skinny_split(0), rt.set_chain_skinny(0), rt.set_skinny_split(0))" % ROOT)
    for text, want in (("4", 4), ("17", 0), ("-1", 0)):
        env = dict({k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}, TPP_HIP_CHAIN_SKINNY_SPLIT=text)
        assert subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=120).strip().splitlines()[-1] == "[0, 0, 0] %d 0 0" % want
