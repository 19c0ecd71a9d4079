"""CPU check of the exactness precondition of tests/test_chain_widths_ragged_gpu.py's exact-input case: for every exact-input vector the GPU
file uses - every tile, B image, m and chain of chain_widths_ragged_worker.specs, with the GPU file's seeds - the oracle's output of every
layer equals the fp64 result rounded once (what chain_widths_worker.check_exact asks before it compares bits). It runs without a GPU, so
the GPU run cannot discover a badly chosen input: the chains are built with the device upload replaced by the host array."""
import numpy as np
import pytest

import chain_widths_worker
from chain_edge_worker import GUARD_ROWS, orc, pkg
from chain_widths_ragged_worker import specs


@pytest.fixture(scope="module")
def rt():
    pkg.build()
    return pkg.get_runtime()


@pytest.mark.parametrize("image", [2, 0, 4])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_the_oracle_s_output_is_the_fp64_result_rounded_once(rt, monkeypatch, t, image):
    monkeypatch.setattr(chain_widths_worker, "dev", lambda a: a)  # no device: the operands stay on the host
    seen = 0
    for mi in (0, 1):
        seed = 1000 * t + 100 * image + 10000 * mi  # (the GPU file's)
        for i, (name, m, ns, ks, brs) in enumerate(specs(t, mi)):
            ch = chain_widths_worker.WidthsChain(rt, image, m, ns, ks, brs, seed + i, exact=True)
            ref, prev = ch.oracle(), ch.x
            v, rows = image or 1, m + GUARD_ROWS
            for l in range(ch.L):
                K, n = ks[l] * brs[l], ns[l]
                xin = orc.bf16_to_f32(prev).reshape(rows, -1)[:m, :K].astype(np.float64)
                w = orc.bf16_to_f32(ch.W[l]).reshape(-1, ch.ldb[l], v)[:K // v, :n, :].transpose(0, 2, 1).reshape(K, n).astype(np.float64)
                f64 = np.maximum(xin @ w + orc.bf16_to_f32(ch.b[l])[:n].astype(np.float64)[None, :], 0)
                got = ref[l].reshape(rows, ch.ldc[l])[:m, :n]
                assert np.array_equal(orc.f32_to_bf16(f64.astype(np.float32).reshape(-1)).reshape(m, n), got), "%s, tile %d image %d m %d layer %d: not exact" % (name, t, image, m, l)
                # and exact in the strong sense: the fp64 sums are integers an fp32 accumulator holds whatever the order of the sums
                assert np.array_equal(f64, np.rint(f64)) and np.abs(xin).max() * np.abs(w).sum(axis=0).max() + 40 < 2 ** 24
                prev = ref[l]
            assert (got & 0x7fff).max() > 0, "%s: the last layer is all zeros" % name
            seen += 1
    assert seen == 27
