"""Worker of tests/test_call_switches_gpu.py, and the rows and helpers it shares with that test and with tests/test_gemm_call_switches.py (which
imports ROWS on a machine without a GPU: nothing here touches the library before a function is called). As a program (its own process: the
eight modes and strict mode come from the environment, read when the library is loaded): the named rows, one call each on random operands.
Prints one JSON line: the modes as the library read them, and per row the kernel text, a digest of the result's bits and the counters
that moved.
  call_switches_worker.py <seed> <row label> ..."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 1, 2

# the eight mode switches (Runtime.set_<name>, Runtime.<name>_stats, TPP_HIP_<NAME>) and the value each has in a context
SWITCHES = ["dma256_edge", "edge_tiles", "edge_k", "edge_k_bf16", "edge_k8_bf16", "dma256_images", "tail_split", "f32_halves"]
CONTEXTS = {
    "rule": dict(dma256_edge=1, edge_tiles=2, edge_k=1, edge_k_bf16=1, edge_k8_bf16=1, dma256_images=1, tail_split=1, f32_halves=1),
    "eligible": dict(dma256_edge=2, edge_tiles=2, edge_k=1, edge_k_bf16=1, edge_k8_bf16=1, dma256_images=2, tail_split=2, f32_halves=2),
}
OFF = dict.fromkeys(SWITCHES, 0)
# what the refinement that moves <name>_stats reads (gemm_plan.h, above plan_gemm_call)
READS = {"dma256_edge": ["dma256_edge"], "edge_tiles": ["edge_tiles"], "edge_k": ["edge_k", "edge_tiles"], "edge_k_bf16": ["edge_k_bf16", "edge_tiles"],
         "edge_k8_bf16": ["edge_k8_bf16", "edge_tiles"], "dma256_images": ["dma256_images"], "tail_split": ["tail_split"], "f32_halves": ["f32_halves"]}
CHAIN_COUNTERS = ["chain_dma256", "chain_edge", "chain_ragged", "chain_widths", "chain_width_rounds", "chain_widths_ragged", "chain_rounds"]
SFX = {2: "", 0: "_flatb", 4: "_vnni4"}   # B image of tests/dma256_images_worker.py Case (2 VNNI-2, 0 flat, 4 VNNI-4) -> kernel name
TAG = {2: "v2", 0: "flat", 4: "v4"}


def row(label, dt, m, n, k, br=1, image=None, force=None, vc=False, c8=False, split=None, rule=(None, ""), eligible=None, golden=None):
    """one call: `rule` / `eligible` = (the switch whose counter moves or None, the text xsmm_hip_last_refined_kernel reports) with every switch on"""
    return dict(label=label, dt=dt, m=m, n=n, k=k, br=br, image=image, force=force, vc=vc, c8=c8, split=split,
                expect={"rule": rule, "eligible": rule if eligible is None else eligible}, golden=golden or label)


def _rows():
    r = []
    for im in (2, 0, 4):
        t, lw, d = TAG[im], "brgemm_bf16_lw%s<32x64,k2>" % SFX[im], "brgemm_bf16_dma%s<256x256>, edge tiles" % SFX[im]
        r.append(row("gpu:d256e-264x256x32-" + t, BF16, 264, 256, 32, image=im, eligible=("dma256_edge", d)))
        # eligible for three switches at once: the 256x256 tile wins; under its rule (too few tiles) the ragged-k launch on edge tiles does
        r.append(row("gpu:d256e-256x264x96-" + t, BF16, 256, 264, 96, image=im, rule=("edge_k_bf16", lw + ", edge tiles, ragged k"), eligible=("dma256_edge", d)))
        # k % 32 != 0: refused by the 256x256 edge tiles
        r.append(row("gpu:k8-fallthrough-264x264x72-" + t, BF16, 264, 264, 72, image=im, rule=("edge_k8_bf16", lw + ", edge tiles, ragged k, half step")))
        r.append(row("gpu:bf16-edge-40x72x64-" + t, BF16, 40, 72, 64, image=im, rule=("edge_tiles", lw + ", edge tiles")))
        r.append(row("gpu:k8-64x64x72-" + t, BF16, 64, 64, 72, image=im, rule=("edge_k8_bf16", lw + ", ragged k, half step")))
        r.append(row("gpu:bf16-both-40x72x72-" + t, BF16, 40, 72, 72, image=im, rule=("edge_k8_bf16", lw + ", edge tiles, ragged k, half step")))
        r.append(row("gpu:bf16-both16-40x72x80-" + t, BF16, 40, 72, 80, image=im, rule=("edge_k_bf16", lw + ", edge tiles, ragged k")))
    r.append(row("gpu:kedge-64x64x80-flat", BF16, 64, 64, 80, image=0, rule=("edge_k_bf16", "brgemm_bf16_lw_flatb<32x64,k2>, ragged k")))
    r.append(row("gpu:kedge-64x64x80-v4", BF16, 64, 64, 80, image=4, rule=("edge_k_bf16", "brgemm_bf16_lw_vnni4<32x64,k2>, ragged k")))
    # VNNI-2 is dispatched on the 32x32 K-split kernel: past the gate (br * k >= 1024) at br = 13, inside it at br = 1
    r.append(row("gpu:kedge-64x64x80-v2-br13", BF16, 64, 64, 80, br=13, image=2, rule=("edge_k_bf16", "brgemm_bf16_lw<32x64,k2>, ragged k")))
    r.append(row("gpu:kedge-gated-64x64x80-v2-br1", BF16, 64, 64, 80, image=2))
    r.append(row("gpu:images-256x256x64-flat", BF16, 256, 256, 64, image=0, eligible=("dma256_images", "brgemm_bf16_dma_flatb<256x256>")))
    r.append(row("gpu:images-256x256x64-v4", BF16, 256, 256, 64, image=4, eligible=("dma256_images", "brgemm_bf16_dma_vnni4<256x256>")))
    r.append(row("gpu:f32-edge-40x36x64", F32, 40, 36, 64, rule=("edge_tiles", "brgemm_f32_lw<32x32,k4>, edge tiles")))
    r.append(row("gpu:f32-kedge-64x64x72", F32, 64, 64, 72, rule=("edge_k", "brgemm_f32_lw<32x32,k4>, ragged k")))
    r.append(row("gpu:f32-both-40x36x72", F32, 40, 36, 72, rule=("edge_k", "brgemm_f32_lw<32x32,k4>, edge tiles, ragged k")))
    # the smallest cases of tests/test_f32_halves_gpu.py and tests/test_tail_split_gpu.py; the rules ask for a tile per compute unit / a saving
    r.append(row("gpu:halves-64x64x64-f6", F32, 64, 64, 64, force=6, eligible=("f32_halves", "")))
    r.append(row("gpu:split-64x128x64-f6-br4", F32, 64, 128, 64, br=4, force=6, split=2, rule=(None, "brgemm_f32_lw<64x64,k2>, split")))
    # 16 x (CUs / 16 + 1) tiles of 32x32 + K4: n comes from the device (tail_shape); the golden row is the one of 256 compute units
    r.append(row("gpu:tail-512xCUs-f9-br4", F32, 512, None, 64, br=4, force=9, eligible=("tail_split", "brgemm_f32_lw<32x32,k4>, tail split"),
                 golden="tail-512x544-f9-br4"))
    # calls every switch leaves alone
    r.append(row("gpu:stays-128x128x64-f32", F32, 128, 128, 64))
    r.append(row("gpu:stays-128x128x64-v2", BF16, 128, 128, 64, image=2))
    r.append(row("gpu:stays-128x128x64-flat", BF16, 128, 128, 64, image=0))
    r.append(row("gpu:stays-forced-256x256x64-flat-f25", BF16, 256, 256, 64, image=0, force=25))
    r.append(row("gpu:stays-forced-40x36x64-f32-f8", F32, 40, 36, 64, force=8))
    r.append(row("gpu:stays-vc-264x256x32-v2", BF16, 264, 256, 32, image=2, vc=True))
    r.append(row("gpu:stays-c8-264x256x32-v2", BF16, 264, 256, 32, image=2, c8=True))
    r.append(row("gpu:stays-c8-40x36x64-f32", F32, 40, 36, 64, c8=True))
    return r


ROWS = _rows()
BY_LABEL = {r["label"]: r for r in ROWS}
# the rows the child process repeats. Each is larger than 64 x 64: in strict mode a single invoke of at most 64 x 64 outputs runs on the grouped
# launcher with a work list of one (rt_invoke.h), which plan_gemm_group plans - no single-call switch reaches it
ENV_ROWS = ["gpu:d256e-256x264x96-flat", "gpu:k8-fallthrough-264x264x72-v4", "gpu:tail-512xCUs-f9-br4"]


def runtime():
    sys.path.insert(0, ROOT)
    return importlib.import_module("tpp-mlir_amd").get_runtime()


def set_modes(rt, values):
    """sets all eight modes; returns what they were"""
    return {s: getattr(rt, "set_" + s)(values[s]) for s in SWITCHES}


def counters(rt):
    return {s: getattr(rt, s + "_stats")()[0] for s in SWITCHES + CHAIN_COUNTERS}


def moved(before, after):
    return {s: after[s] - before[s] for s in before if after[s] != before[s]}


def tail_shape():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus % 16 == 0, "%d compute units do not divide into 16 tile rows" % cus
    return (cus // 16 + 1) * 32


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


class F32Case:
    """One whole-layer f32 call through tests/edge_tiles_worker.py layer_call: packed operands, a band of a bit pattern in front of and behind
    the C window, NaN in the window under beta 0. exact: small integers (tests/exact_data.py), else uniform [-1, 1). c8: C starts 8 bytes off
    a 16-byte boundary."""
    GUARD = 64

    def __init__(self, m, n, k, br, seed, exact=False, beta0=False, c8=False):
        import exact_data as ed
        self.m, self.n, self.k, self.br, self.K = m, n, k, br, k * br
        self.beta0, self.bias, self.relu = beta0, beta0, beta0
        rng = np.random.default_rng(seed)
        sizes = (m * self.K + 8, self.K * n + 8, m * n, n + 8)
        if exact:
            ra, rb, rc = ed.exact_ranges(F32, self.K)
            self.A, self.B, c0, self.D = (ed.exact_fill(rng, s, F32, r) for s, r in zip(sizes, (ra, rb, rc, rc)))
        else:
            self.A, self.B, c0, self.D = (rng.uniform(-1, 1, s).astype(np.float32) for s in sizes)
        self.c_off = self.GUARD + (2 if c8 else 0)
        bits = (np.arange(self.c_off + m * n + self.GUARD, dtype=np.uint64) * 2654435761 + 12345).astype(np.uint32)
        self.C = bits.view(np.float32).copy()
        self.win = self.c_off + np.arange(m * n)
        self.C[self.win] = np.nan if beta0 else c0

    def fp64(self):
        """the result in fp64, rounded once to f32 (exact inputs: nothing is rounded)"""
        m, n, k = self.m, self.n, self.k
        acc = np.zeros((m, n)) if self.beta0 else self.C[self.win].astype(np.float64).reshape(m, n)
        A, B = self.A[:m * self.K].astype(np.float64).reshape(m, self.K), self.B[:self.K * n].astype(np.float64).reshape(self.K, n)
        for b in range(self.br):
            acc = acc + A[:, b * k:(b + 1) * k] @ B[b * k:(b + 1) * k, :]
        if self.bias:
            acc = acc + self.D[:n].astype(np.float64)[None, :]
        if self.relu:
            acc = np.maximum(acc, 0)
        return acc.astype(np.float32).reshape(-1)

    def oracle(self):
        from oracle import pyoracle as orc
        ref = self.C.copy()
        orc.fused_brgemm(F32, self.m, self.n, self.k, self.K, self.n, self.n, self.k, self.k * self.n, 4 if self.beta0 else 0, 0, 5 if self.relu else 0,
                         4 if self.bias else 0, 1 if self.bias else 0, self.A, 0, self.B, 0, ref, self.c_off, self.D, 0, self.br)
        return ref

    def run(self, rt, force=None):
        from edge_tiles_worker import layer_call
        got, refined = layer_call(rt, self.m, self.n, self.K, self.A, self.B, self.C, self.D, k=self.k, beta0=self.beta0, bias=self.bias, relu=self.relu,
                                  offs=(0, 0, self.c_off, 0), force=force)
        return got, refined

    def outside_untouched(self, got):
        mask = np.ones(self.C.size, bool)
        mask[self.win] = False
        return np.array_equal(got.view(np.uint32)[mask], self.C.view(np.uint32)[mask])


class VcCase:
    """One whole-layer bf16 call with a VNNI-2 C through tests/edge_tiles_bf16_worker.py layer_call (packed operands, uniform values): compared
    with the same call under other modes only."""

    def __init__(self, r, seed):
        from edge_tiles_bf16_worker import operands
        self.r, self.K = r, r["k"] * r["br"]
        self.ops = operands(r["m"], r["n"], self.K, seed)
        self.win = np.arange(r["m"] * r["n"])

    def run(self, rt, force=None):
        from edge_tiles_bf16_worker import layer_call
        r = self.r
        return layer_call(rt, r["image"], r["m"], r["n"], self.K, *self.ops, k=r["k"], force=force, vnni_c=True)


def make_case(r, seed, exact=False, beta0=False):
    """the operands of a row (tests/dma256_images_worker.py Case for bf16: strided, moved base pointers, NaN in every gap, a bit pattern around C)"""
    n = tail_shape() if r["n"] is None else r["n"]
    if r["vc"]:
        return VcCase(r, seed)
    if r["dt"] == F32:
        return F32Case(r["m"], n, r["k"], r["br"], seed, exact=exact, beta0=beta0, c8=r["c8"])
    from dma256_images_worker import Case
    return Case(r["image"], r["m"], n, r["k"], r["br"], seed, exact=exact, beta0=beta0, bias=beta0, relu=beta0, offs=(8, 16, 4, 4) if r["c8"] else None)


def run_case(rt, r, case):
    """the row's call under whatever modes are set; returns (the whole C buffer, the kernel text, the counters that moved)"""
    prev = rt.force_split(r["split"]) if r["split"] is not None else None
    before = counters(rt)
    try:
        out = case.run(rt, force=r["force"])
        rt.synchronize()
    finally:
        if r["split"] is not None:
            rt.force_split(prev)
    return out[0], out[1], moved(before, counters(rt))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    rt = runtime()
    modes = set_modes(rt, OFF)   # what the library read from the environment
    set_modes(rt, modes)
    out = {"modes": modes, "strict": rt.get_strict(), "rows": {}}
    for label in sys.argv[2:]:
        r = BY_LABEL[label]
        got, text, mv = run_case(rt, r, make_case(r, int(sys.argv[1])))
        out["rows"][label] = {"kernel": text, "digest": digest(got), "moved": mv}
    print(json.dumps(out))
