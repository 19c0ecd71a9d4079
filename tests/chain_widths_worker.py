"""Helper of tests/test_chain_widths_gpu.py, and its worker. WidthsChain lays a mixed-width bf16 layer chain out as chain_edge_worker.RaggedChain
does, with per-layer n, ldb and ldc. As a program (its own process: strict mode is chosen before anything is queued; the switch comes from
the environment): one mixed-width chain whose calls are dispatched on DIFFERENT tiles, under TPP_HIP_STRICT=1 and TPP_HIP_CHAIN_WIDTHS=1 through
xsmm_hip_fused_brgemm_chain_invoke. Prints one JSON line: the settings as the library read them, whether the chain ran as one launch, the
counter and a digest of every layer's bits.
  chain_widths_worker.py <image: 2 VNNI-2, 0 flat, 4 VNNI-4> <m> <seed> <n0,n1,..> <tile of call 0,tile of call 1,..>"""
import json
import sys

import numpy as np

from chain_edge_worker import BASE, BF16, F32, GAP, GUARD_ROWS, NAN, SENTINEL, VB, b_image, dev, digest, orc, pkg


class WidthsChain:
    """layer l has ns[l] columns on m rows and reads brs[l] batch elements of ks[l] columns (stride_a = ks[l]: along k) of its predecessor's
    output (ks[l] * brs[l] <= ns[l - 1]). Every buffer carries GAP columns beyond its last one and GUARD_ROWS rows behind its last row: NaN
    around the layer-0 input, the weights and the bias rows; SENTINEL around every output, NaN inside it. tiles: the loader-wave tile every
    call (or call l, a list) is dispatched on with force_variant; None = the planner's own choice."""

    def __init__(self, rt, image, m, ns, ks, brs, seed, exact=False, dtype=BF16, tiles=None, ms=None):
        self.rt, self.image, self.m, self.ns, self.ks, self.brs, self.dtype = rt, image, m, list(ns), list(ks), list(brs), dtype
        self.L = len(ns)
        assert len(ks) == len(brs) == self.L and all(ks[l] * brs[l] <= ns[l - 1] for l in range(1, self.L))
        rng = np.random.default_rng(seed)
        self.ld_in = [ks[0] * brs[0] + GAP] + [ns[l - 1] + GAP for l in range(1, self.L)]  # leading dimension of layer l's A operand
        self.ldb = [n + GAP for n in ns]
        self.ldc = self.ldb
        f32 = dtype == F32
        self.np_t = np.float32 if f32 else np.uint16
        nan, self.sentinel = (np.float32(np.nan), np.float32(1.5)) if f32 else (NAN, SENTINEL)
        store = (lambda v: v.astype(np.float32)) if f32 else (lambda v: orc.f32_to_bf16(v.astype(np.float32)))
        v = 1 if (f32 or not image) else image
        self.W, self.b = [], []
        for l in range(self.L):
            K, n = ks[l] * brs[l], ns[l]
            if exact:  # weights in {-1, 0, 1}, about 4 nonzeros per column: integer activations stay small integers at every layer
                q = min(1.0, 4.0 / K)
                w = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=K * n, p=[q / 2, 1 - q, q / 2])
                b = rng.integers(-40, 41, n).astype(np.float32)
            else:
                w, b = rng.uniform(-0.25, 0.25, K * n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
            W = np.full((K // v + GUARD_ROWS, self.ldb[l], v), nan, self.np_t)  # [K / v][ldb][v]: flat (v = 1), VNNI-2, VNNI-4
            W[:K // v, :n, :] = store(w).reshape(K // v, n, v)
            D = np.full(n + GAP, nan, self.np_t)
            D[:n] = store(b)
            self.W.append(W.reshape(-1))
            self.b.append(D)
        x = rng.integers(-15, 16, m * ks[0] * brs[0]) if exact else rng.uniform(-1, 1, m * ks[0] * brs[0])
        X = np.full((m + GUARD_ROWS, self.ld_in[0]), nan, self.np_t)
        X[:m, :ks[0] * brs[0]] = store(np.asarray(x, np.float32)).reshape(m, -1)
        self.x = X.reshape(-1)
        self.out_templates = []
        for n in ns:
            out = np.full((m + GUARD_ROWS, n + GAP), self.sentinel, self.np_t)
            out[:m, :n] = nan
            self.out_templates.append(out.reshape(-1))
        self.flags = 4 | (VB if (image and not f32) else 0)
        self.handles = []
        with b_image(rt, 0 if f32 else image):
            try:
                for l in range(self.L):
                    t = tiles[l] if isinstance(tiles, (list, tuple)) else tiles
                    rt.force_variant(-1 if t is None else BASE[image] + t)
                    self.handles.append(rt.fused_brgemm_dispatch(dtype, ms[l] if ms else m, ns[l], ks[l], self.ld_in[l], self.ldb[l], self.ldc[l], ks[l], ks[l] * self.ldb[l],
                                                                 self.flags, 0, 5, 4, 1))
            finally:
                rt.force_variant(-1)
        self.dx, self.dW, self.db = dev(self.x), [dev(w) for w in self.W], [dev(b) for b in self.b]
        self.d_templates = [dev(o) for o in self.out_templates]

    def outputs(self):
        return [t.clone() for t in self.d_templates]

    def refill(self, outs):
        for o, t in zip(outs, self.d_templates):
            o.copy_(t)

    def calls(self, outs):
        cur, c = self.dx, []
        for l in range(self.L):
            c.append((self.handles[l], cur, 0, self.dW[l], 0, outs[l], 0, self.db[l], 0, self.brs[l]))
            cur = outs[l]
        return c

    def one_by_one(self, outs):
        for c in self.calls(outs):
            self.rt.fused_brgemm(self.dtype, *c)

    def host(self, outs):
        self.rt.synchronize()
        return [o.cpu().numpy().view(self.np_t) for o in outs]

    def oracle(self):
        """every layer by the oracle, fed the oracle's previous layer; same buffers, same guards"""
        cur, outs = self.x, []
        with b_image(self.rt, 0 if self.dtype == F32 else self.image):
            for l in range(self.L):
                out = self.out_templates[l].copy()
                orc.fused_brgemm(self.dtype, self.m, self.ns[l], self.ks[l], self.ld_in[l], self.ldb[l], self.ldc[l], self.ks[l], self.ks[l] * self.ldb[l], self.flags, 0, 5, 4, 1,
                                 cur, 0, self.W[l], 0, out, 0, self.b[l], 0, self.brs[l])
                outs.append(out)
                cur = out
        return outs

    def check_windows(self, got, rows=None):
        """the guard rows and gap columns of every output still hold the sentinel, no NaN inside any output, and the operands are as uploaded"""
        for l, g in enumerate(got):
            m, n = (rows[l] if rows else self.m), self.ns[l]
            g2 = g.reshape(self.m + GUARD_ROWS, self.ldc[l])
            # (rows behind a call's own m are as the template has them: NaN inside the buffer's m x n, the sentinel in the guard rows)
            assert np.array_equal(g2[m:, :], self.out_templates[l].reshape(g2.shape)[m:, :], equal_nan=True), "layer %d: rows behind row m were written" % l
            assert np.array_equal(g2[:, n:], np.full_like(g2[:, n:], self.sentinel)), "layer %d: columns beyond n were written" % l
            inside = g2[:m, :n]
            nans = np.isnan(inside) if self.dtype == F32 else ((inside & 0x7f80) == 0x7f80) & ((inside & 0x7f) != 0)
            assert not nans.any(), "layer %d: %d NaNs inside the output (an unwritten element, or a guard was read)" % (l, int(nans.sum()))
        assert np.array_equal(self.dx.cpu().numpy().view(self.np_t), self.x, equal_nan=self.dtype == F32)
        for l in range(self.L):
            assert np.array_equal(self.dW[l].cpu().numpy().view(self.np_t), self.W[l], equal_nan=True), "layer %d: the weights were written" % l


def check_exact(ch, got):
    """every layer bit for bit the oracle's (fed the oracle's previous layer), the exactness precondition checked per layer: the oracle's
    output is the fp64 result rounded once"""
    ref, prev = ch.oracle(), ch.x
    v = ch.image or 1
    rows = ch.m + GUARD_ROWS
    for l in range(ch.L):
        K, n = ch.ks[l] * ch.brs[l], ch.ns[l]
        xin = orc.bf16_to_f32(prev).reshape(rows, -1)[:ch.m, :K].astype(np.float64)
        w = orc.bf16_to_f32(ch.W[l]).reshape(-1, ch.ldb[l], v)[:K // v, :n, :].transpose(0, 2, 1).reshape(K, n).astype(np.float64)
        f64 = np.maximum(xin @ w + orc.bf16_to_f32(ch.b[l])[:n].astype(np.float64)[None, :], 0)
        r2, g2 = ref[l].reshape(rows, ch.ldc[l]), got[l].reshape(rows, ch.ldc[l])
        assert np.array_equal(orc.f32_to_bf16(f64.astype(np.float32).reshape(-1)).reshape(ch.m, n), r2[:ch.m, :n]), "layer %d not exact" % l
        bad = g2 != r2
        assert not bad.any(), "layer %d: %d elements differ from the oracle, first at (row, column) %s" % (l, int(bad.sum()), tuple(np.argwhere(bad)[0]))
        prev = ref[l]


if __name__ == "__main__":
    image, m, seed = (int(x) for x in sys.argv[1:4])
    ns, tiles = [int(x) for x in sys.argv[4].split(",")], [int(x) for x in sys.argv[5].split(",")]
    rt = pkg.get_runtime()
    was_async = rt.set_async(True)
    out = {"strict": rt.get_strict(), "chain_widths_from_env": rt.set_chain_widths(1)}
    ch = WidthsChain(rt, image, m, ns, [192] + ns[:-1], [1] * len(ns), seed, tiles=tiles)
    outs = ch.outputs()
    out["ran_as_one"] = bool(rt.fused_brgemm_chain(BF16, ch.calls(outs)))
    got = ch.host(outs)
    ch.check_windows(got)
    out["digests"] = [digest(g) for g in got]
    out["chain_widths_stats"] = list(rt.chain_widths_stats())
    rt.set_chain_widths(0), rt.set_async(was_async)
    print(json.dumps(out))
