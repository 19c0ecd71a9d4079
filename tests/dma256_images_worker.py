"""Worker of tests/test_dma256_images_gpu.py, and the case builder the test shares with it. As a program (its own process: the mode comes
from the environment, read when the library is loaded): one whole-layer bf16 call with a flat or VNNI-4 B under TPP_HIP_DMA256_IMAGES=<mode>,
three times on the same data. Prints one JSON line: the mode as the library read it, the kernel each call reported, the counters and a
digest of each result's bits.
  dma256_images_worker.py <image: 0 flat, 4 VNNI-4> <m> <n> <k> <br> <seed>"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("tpp-mlir_amd")
import exact_data as ed  # noqa: E402
from edge_tiles_bf16_worker import BF16, VB, b_image, digest  # noqa: E402,F401
from oracle import pyoracle as orc  # noqa: E402


class Case:
    """One whole-layer bf16 call: br batch elements, each k wide, of a row-major A and of B in image `image` (0 flat, 2 / 4 VNNI). Strided:
    a gap of 8 columns behind every batch element of an A row and 8 more behind the row, 4 k-rows between the batch elements of B and 8
    columns behind its rows, 16 behind the rows of C, every base pointer moved (by 16, 32, 16 and 8 bytes) - the batch strides are not the
    packed ones. exact: small integers (every partial sum an integer an f32 holds), else uniform A in [-1, 1), B in [-0.5, 0.5).
    poison: NaN in everything the descriptor does not name - gap columns, the rows between batch elements, guard rows, the C window under
    beta 0 - and a bit pattern around the C window."""

    def __init__(self, image, m, n, k, br, seed, exact=False, beta0=False, bias=True, relu=True, strided=True, poison=True, offs=None):
        self.image, self.m, self.n, self.k, self.br = image, m, n, k, br
        self.beta0, self.bias, self.relu = beta0, bias, relu
        self.v = image or 1
        nb = max(br, 1)
        if strided:
            self.lda, self.sa, self.ldb, self.ldc, self.offs = nb * (k + 8) + 8, k + 8, n + 8, n + 16, (8, 16, 8, 4)
            self.sb = (k + 4) * self.ldb
        else:
            self.lda, self.sa, self.ldb, self.ldc, self.sb, self.offs = k * nb, k, n, n, k * n, (0, 0, 0, 0)
        if offs is not None:
            self.offs = offs
        o = self.offs
        sizes = (o[0] + (nb - 1) * self.sa + m * self.lda + 8, o[1] + (nb - 1) * self.sb + k * self.ldb + 2 * self.ldb + 8, o[2] + m * self.ldc + 8, o[3] + n + 8)
        rng = np.random.default_rng(seed)
        if exact:
            ra, rb, rc = ed.exact_ranges(BF16, k * nb)
            assert k * nb * ra * rb + 2 * rc * (1 + 2.0 ** -8) < 2 ** 24
            self.A, self.B, self.C, self.D = (ed.exact_fill(rng, s, BF16, r) for s, r in zip(sizes, (ra, rb, rc, rc)))
        else:
            self.A, self.B, self.C, self.D = (orc.f32_to_bf16(rng.uniform(-s_, s_, s).astype(np.float32)) for s, s_ in zip(sizes, (1, 0.5, 1, 1)))
        ii, jj = np.arange(m)[:, None], np.arange(n)[None, :]
        self.win = (o[2] + ii * self.ldc + jj).reshape(-1)
        if poison:
            la, lb, _, ld_ = ed.live_masks(sizes, m, n, k, nb, self.lda, self.ldb, self.ldc, self.sa, self.sb, o, vnni=bool(image), v=self.v, beta0=beta0, bias=bias)
            for arr, lv in zip((self.A, self.B, self.D), (la, lb, ld_)):
                arr[~lv] = ed.BF16_NAN
            keep = self.C[self.win].copy()
            self.C[:] = (np.arange(sizes[2], dtype=np.uint32) * 40503 + 12345).astype(np.uint16)  # the bit pattern around C
            self.C[self.win] = ed.BF16_NAN if beta0 else keep

    def flags(self):
        return (4 if self.beta0 else 0) | (VB if self.image else 0)

    def b_index(self, b, kk, jj):
        return self.offs[1] + b * self.sb + ed.b_live_index(kk, jj, self.ldb, bool(self.image), self.v)

    def fp64(self):
        """the result in fp64, rounded ONCE to bf16 (exact inputs: every intermediate is an integer below 2^24, so the f32 step rounds nothing)"""
        m, n, k, o = self.m, self.n, self.k, self.offs
        ii, kk, jj = np.arange(m)[:, None], np.arange(k)[None, :], np.arange(n)[None, :]
        acc = np.zeros((m, n)) if self.beta0 else orc.bf16_to_f32(self.C[self.win]).astype(np.float64).reshape(m, n)
        for b in range(self.br):
            a = orc.bf16_to_f32(self.A[(o[0] + b * self.sa + ii * self.lda + kk).reshape(-1)]).astype(np.float64).reshape(m, k)
            w = orc.bf16_to_f32(self.B[self.b_index(b, np.arange(k)[:, None], jj).reshape(-1)]).astype(np.float64).reshape(k, n)
            acc = acc + a @ w
        if self.bias:
            acc = acc + orc.bf16_to_f32(self.D[o[3]:o[3] + n]).astype(np.float64)[None, :]
        if self.relu:
            acc = np.maximum(acc, 0)
        return orc.f32_to_bf16(acc.astype(np.float32).reshape(-1))

    def oracle(self):
        """the whole C buffer after the oracle's call"""
        ref, o = self.C.copy(), self.offs
        with _oracle_image(self.image):
            if self.bias or self.relu:
                orc.fused_brgemm(BF16, self.m, self.n, self.k, self.lda, self.ldb, self.ldc, self.sa, self.sb, self.flags(), 0, 5 if self.relu else 0,
                                 4 if self.bias else 0, 1 if self.bias else 0, self.A, o[0], self.B, o[1], ref, o[2], self.D, o[3], self.br)
            else:
                orc.brgemm(BF16, self.m, self.n, self.k, self.lda, self.ldb, self.ldc, self.sa, self.sb, self.flags(), self.A, o[0], self.B, o[1], ref, o[2], self.br)
        return ref

    def dispatch(self, rt, force=None):
        with b_image(rt, self.image):
            if force is not None:
                rt.force_variant(force)
            try:
                if self.bias or self.relu:
                    return rt.fused_brgemm_dispatch(BF16, self.m, self.n, self.k, self.lda, self.ldb, self.ldc, self.sa, self.sb, self.flags(), 0,
                                                    5 if self.relu else 0, 4 if self.bias else 0, 1 if self.bias else 0)
                return rt.brgemm_dispatch(BF16, self.m, self.n, self.k, self.lda, self.ldb, self.ldc, self.sa, self.sb, self.flags())
            finally:
                if force is not None:
                    rt.force_variant(-1)

    def device(self):
        import torch
        return [torch.from_numpy(x.view(np.int16).copy()).cuda() for x in (self.A, self.B, self.C, self.D)]

    def run(self, rt, force=None, br=None):
        """on device copies; returns the whole C buffer after the call (uint16), what xsmm_hip_last_refined_kernel reported and the
        descriptor's own kernel name"""
        h = self.dispatch(rt, force)
        dA, dB, dC, dD = self.device()
        o, br = self.offs, self.br if br is None else br
        if self.bias or self.relu:
            rt.fused_brgemm(BF16, h, dA, o[0], dB, o[1], dC, o[2], dD, o[3], br)
        else:
            rt.brgemm(BF16, h, dA, o[0], dB, o[1], dC, o[2], br)
        refined = rt.last_refined_kernel()
        return dC.cpu().numpy().view(np.uint16), refined, rt.kernel_name(h)

    def outside_untouched(self, got):
        mask = np.ones(self.C.size, bool)
        mask[self.win] = False
        return np.array_equal(got[mask], self.C[mask])

    def as_vnni2(self):
        """the same call with its flat B packed into VNNI-2 pair-rows, same leading dimension and strides (needs an even k + gap)"""
        assert self.image == 0 and self.k % 2 == 0 and (self.sb // self.ldb) % 2 == 0
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.image, c.v, c.B = 2, 2, self.B.copy()
        kk, jj = np.arange(self.k)[:, None], np.arange(self.n)[None, :]
        for b in range(self.br):
            c.B[c.b_index(b, kk, jj).reshape(-1)] = self.B[self.b_index(b, kk, jj).reshape(-1)]
        return c


class _oracle_image:
    def __init__(self, image):
        self.image = image

    def __enter__(self):
        self.old = orc.set_vnni_factor(self.image) if self.image else None

    def __exit__(self, *a):
        if self.image:
            orc.set_vnni_factor(self.old)


if __name__ == "__main__":
    image, m, n, k, br, seed = (int(x) for x in sys.argv[1:7])
    rt = pkg.get_runtime()
    mode = rt.set_dma256_images(0)  # what the library read from the environment
    rt.set_dma256_images(mode)
    out = {"from_env": mode, "kernels": [], "digests": []}
    case = Case(image, m, n, k, br, seed)
    for _ in range(3):
        got, refined, _ = case.run(rt)
        out["kernels"].append(refined)
        out["digests"].append(digest(got))
    out["stats"] = list(rt.dma256_images_stats())
    print(json.dumps(out))
