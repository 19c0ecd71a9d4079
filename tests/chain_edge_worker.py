"""Worker of tests/test_chain_edge_gpu.py, and the chain helpers the test shares with it. As a program (its own process: strict mode is chosen
before anything is queued; the switch and the forced tile come from the environment): one ragged-m bf16 layer chain under TPP_HIP_STRICT=1,
TPP_HIP_CHAIN_EDGE=1 and TPP_HIP_EDGE_TILES=<20 + t> through xsmm_hip_fused_brgemm_chain_invoke. Prints one JSON line: the settings as the
library read them, whether the chain ran as one launch, the counters and a digest of every layer's bits.
  chain_edge_worker.py <t> <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <n> <seed>"""
import contextlib
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("tpp-mlir_amd")
from oracle import pyoracle as orc  # noqa: E402

F32, BF16, VB = 1, 2, 2048
NAN, SENTINEL = 0x7fc0, 0x1234  # bf16 NaN; the bit pattern (a small positive number) behind and beside every output
GUARD_ROWS, GAP = 8, 8
TILE = [(32, 64), (64, 64), (64, 128), (128, 128)]  # set_edge_tiles(20 + t) -> output tile
BASE = {2: 20, 0: 24, 4: 28}                          # B image -> GemmVariant of its 32x64 + K2 tile


@contextlib.contextmanager
def b_image(rt, image):
    """dispatches inside see a VNNI-`image` B operand (0: flat - the factor stays what it is); the runtime's and the oracle's factor"""
    if not image:
        yield
        return
    old, old_o = rt.set_vnni_factor(image), orc.set_vnni_factor(image)
    try:
        yield
    finally:
        rt.set_vnni_factor(old)
        orc.set_vnni_factor(old_o)


def dev(arr):
    import torch
    return torch.from_numpy((arr.view(np.int16) if arr.dtype == np.uint16 else arr).copy()).cuda()


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


class RaggedChain:
    """layers of n columns on m rows: layer l reads br[l] batch elements of k[l] columns (stride_a = k[l]: along k) of its predecessor's
    output. Every buffer carries GAP columns beyond its last one and GUARD_ROWS rows behind its last row: NaN around the layer-0 input,
    the weights (their images' gap columns and guard rows) and the bias rows; SENTINEL around every output, NaN inside it."""

    def __init__(self, rt, image, m, n, ks, brs, seed, exact=False, dtype=BF16, force=None):
        self.rt, self.image, self.m, self.n, self.ks, self.brs, self.dtype = rt, image, m, n, list(ks), list(brs), dtype
        self.L = len(ks)
        rng = np.random.default_rng(seed)
        self.ld_in = [ks[0] * brs[0] + GAP] + [n + GAP] * (self.L - 1)  # leading dimension of layer l's A operand
        self.ldb = self.ldc = n + GAP
        f32 = dtype == F32
        self.np_t = np.float32 if f32 else np.uint16
        nan, self.sentinel = (np.float32(np.nan), np.float32(1.5)) if f32 else (NAN, SENTINEL)
        store = (lambda v: v.astype(np.float32)) if f32 else (lambda v: orc.f32_to_bf16(v.astype(np.float32)))
        v = 1 if (f32 or not image) else image
        self.W, self.b = [], []
        for l in range(self.L):
            K = ks[l] * brs[l]
            if exact:  # weights in {-1, 0, 1}, about 4 nonzeros per column: integer activations stay small integers at every layer
                q = min(1.0, 4.0 / K)
                w = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=K * n, p=[q / 2, 1 - q, q / 2])
                b = rng.integers(-40, 41, n).astype(np.float32)
            else:
                w, b = rng.uniform(-0.25, 0.25, K * n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
            W = np.full((K // v + GUARD_ROWS, self.ldb, v), nan, self.np_t)  # [K / v][ldb][v]: flat (v = 1), VNNI-2, VNNI-4
            W[:K // v, :n, :] = store(w).reshape(K // v, n, v)
            D = np.full(n + GAP, nan, self.np_t)
            D[:n] = store(b)
            self.W.append(W.reshape(-1))
            self.b.append(D)
        x = rng.integers(-15, 16, m * ks[0] * brs[0]) if exact else rng.uniform(-1, 1, m * ks[0] * brs[0])
        X = np.full((m + GUARD_ROWS, self.ld_in[0]), nan, self.np_t)
        X[:m, :ks[0] * brs[0]] = store(np.asarray(x, np.float32)).reshape(m, -1)
        self.x = X.reshape(-1)
        out = np.full((m + GUARD_ROWS, self.ldc), self.sentinel, self.np_t)
        out[:m, :n] = nan
        self.out_template = out.reshape(-1)
        flags = 4 | (VB if (image and not f32) else 0)
        self.handles = []
        with b_image(rt, 0 if f32 else image):
            if force is not None:
                rt.force_variant(force)
            try:
                for l in range(self.L):
                    self.handles.append(rt.fused_brgemm_dispatch(dtype, m, n, ks[l], self.ld_in[l], self.ldb, self.ldc, ks[l], ks[l] * self.ldb, flags, 0, 5, 4, 1))
            finally:
                if force is not None:
                    rt.force_variant(-1)
        self.dx, self.dW, self.db = dev(self.x), [dev(w) for w in self.W], [dev(b) for b in self.b]
        self.d_template = dev(self.out_template)

    def outputs(self):
        return [self.d_template.clone() for _ in range(self.L)]

    def refill(self, outs):
        for o in outs:
            o.copy_(self.d_template)

    def calls(self, outs, dx=None):
        cur, c = self.dx if dx is None else dx, []
        for l in range(self.L):
            c.append((self.handles[l], cur, 0, self.dW[l], 0, outs[l], 0, self.db[l], 0, self.brs[l]))
            cur = outs[l]
        return c

    def one_by_one(self, outs, dx=None):
        for c in self.calls(outs, dx):
            self.rt.fused_brgemm(self.dtype, *c)

    def host(self, outs):
        self.rt.synchronize()
        return [o.cpu().numpy().view(self.np_t) for o in outs]

    def oracle(self):
        """every layer by the oracle, fed the oracle's previous layer; same buffers, same guards"""
        cur, outs = self.x, []
        flags = 4 | (VB if (self.image and self.dtype == BF16) else 0)
        with b_image(self.rt, 0 if self.dtype == F32 else self.image):
            for l in range(self.L):
                out = self.out_template.copy()
                orc.fused_brgemm(self.dtype, self.m, self.n, self.ks[l], self.ld_in[l], self.ldb, self.ldc, self.ks[l], self.ks[l] * self.ldb, flags, 0, 5, 4, 1,
                                 cur, 0, self.W[l], 0, out, 0, self.b[l], 0, self.brs[l])
                outs.append(out)
                cur = out
        return outs

    def check_windows(self, got):
        """the guard rows and gap columns of every output still hold the sentinel, no NaN inside any output, and the operands are as uploaded"""
        for l, g in enumerate(got):
            g2 = g.reshape(self.m + GUARD_ROWS, self.ldc)
            assert np.array_equal(g2[self.m:, :], np.full_like(g2[self.m:, :], self.sentinel)), "layer %d: rows behind row m were written" % l
            assert np.array_equal(g2[:, self.n:], np.full_like(g2[:, self.n:], self.sentinel)), "layer %d: columns beyond n were written" % l
            inside = g2[:self.m, :self.n]
            nans = np.isnan(inside) if self.dtype == F32 else ((inside & 0x7f80) == 0x7f80) & ((inside & 0x7f) != 0)
            assert not nans.any(), "layer %d: %d NaNs inside the output (an unwritten element, or a guard was read)" % (l, int(nans.sum()))
        assert np.array_equal(self.dx.cpu().numpy().view(self.np_t), self.x, equal_nan=self.dtype == F32)


def make_chain(rt, t, image, m, n, seed, br2=False, exact=False, **kw):
    """the test's chain on tile t: three layers, layer 0 of 192 k in one batch element (three chunks, an odd count), later layers k = n; br2:
    two batch elements in every layer, 128 k each in layer 0 and n / 2 (a multiple of 64 for n = 2 BN) in the later ones"""
    if br2:
        return RaggedChain(rt, image, m, n, [128, n // 2, n // 2], [2, 2, 2], seed, exact=exact, **kw)
    return RaggedChain(rt, image, m, n, [192, n, n], [1, 1, 1], seed, exact=exact, **kw)


if __name__ == "__main__":
    t, image, m, n, seed = (int(x) for x in sys.argv[1:6])
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    out = {"strict": rt.get_strict(), "chain_edge_from_env": rt.set_chain_edge(1), "edge_tiles_from_env": rt.set_edge_tiles(20 + t)}
    ch = make_chain(rt, t, image, m, n, seed)
    outs = ch.outputs()
    out["ran_as_one"] = bool(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
    got = ch.host(outs)
    ch.check_windows(got)
    out["digests"] = [digest(g) for g in got]
    out["chain_edge_stats"] = list(rt.chain_edge_stats())
    out["edge_tiles_launches"] = rt.edge_tiles_stats()[0]
    rt.set_chain_edge(0), rt.set_edge_tiles(0), rt.set_async(was_async)
    print(json.dumps(out))
