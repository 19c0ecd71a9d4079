"""Epilogue fold: the element-wise invokes the compiler leaves behind a GEMM tile (brgemm, then binary add / mul / sub / div and / or
unary relu / identity / zero on that tile's output - everything CombineXsmmOp does not fuse) join the queued GEMM group instead of
flushing it. The group runs as its GEMM launch plus one epilogue-program launch and replays that way. Every result must be the bits of
the unfolded invokes (the fold switched off) and of the oracle; the data are exact (small integers) so that the GEMM part is
independent of the kernel family and of the summation order."""
import importlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import exact_data as ed
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
F32, BF16 = 1, 2
ADD, MUL, SUB, DIV = 1, 2, 3, 4
U_IDENTITY, U_ZERO, U_RELU = 1, 2, 5
BCAST = {"none": (0, 0), "row": (1, 2), "col": (4, 8), "scalar": (16, 32)}  # (flag on in0, flag on in1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def rt():
    rt = pkg.get_runtime()
    assert rt.device_count() >= 1
    prev_async = rt.set_async(True)
    prev_q = rt.set_tile_queue(1)
    prev_f = rt.set_fold_epilogue(True)
    yield rt
    rt.synchronize()
    rt.set_fold_epilogue(prev_f)
    rt.set_tile_queue(prev_q)
    rt.set_async(prev_async)


def dev(a):
    import torch
    return torch.from_numpy((a.view(np.int16) if a.dtype == np.uint16 else a).copy()).cuda()


def host(t, dt):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dt == BF16 else a


def store(v, dt):
    v = np.asarray(v, dtype=np.float32)
    return v if dt == F32 else orc.f32_to_bf16(v)


def exact(rng, n, dt, lo=-2, hi=3):
    return store(rng.integers(lo, hi, n), dt)


def special_other(rng, n, dt):
    """the other operand of a post-op with the values that pin the arithmetic: inf, NaN, -0, subnormals, zeros (x / 0)"""
    v = rng.integers(-3, 4, n).astype(np.float32)
    sp = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-40, -1e-40, 3.0, 0.5], dtype=np.float32)
    idx = rng.choice(n, size=max(1, n // 8), replace=False)
    v[idx] = sp[rng.integers(0, len(sp), len(idx))]
    return store(v, dt)


class Layer:
    """an M x N layer of packed tm x tn tiles (A [MB][KB][tm][tk], W [NB][KB][tk][tn], C [MB][NB][tm][tn]), one brgemm invoke per tile,
    each followed by its post-ops: ops = [("binary", kind, bcast, pos) | ("unary", kind)], separate = the chain's outputs go to a
    buffer of their own (else in place)"""

    def __init__(self, rt, dt, M, N, K, tm, tn, tk, ops, separate=False, seed=0, special=False):
        self.rt, self.dt = rt, dt
        self.MB, self.NB, self.KB = M // tm, N // tn, K // tk
        self.tm, self.tn, self.tk = tm, tn, tk
        rng = np.random.default_rng(seed)
        self.A = exact(rng, M * K, dt)
        self.W = exact(rng, K * N, dt)
        nt = self.MB * self.NB
        self.C = np.zeros(nt * tm * tn, dtype=self.A.dtype)
        self.others = [(special_other if special else exact)(rng, nt * tm * tn, dt) for _ in ops]
        self.outs = [np.zeros(nt * tm * tn, dtype=self.A.dtype) for _ in ops]
        self.ops, self.separate = ops, separate
        flags = 4 | (2048 if dt == BF16 else 0)
        self.hg = rt.brgemm_dispatch(dt, tm, tn, tk, tk, tn, tn, tm * tk, tk * tn, flags)
        self.gdisp = (dt, tm, tn, tk, tk, tn, tn, tm * tk, tk * tn, flags)
        self.hops = []
        for op in ops:
            if op[0] == "binary":
                _, kind, bc, pos = op
                f = BCAST[bc][1 - pos]  # the other operand sits in the position the tile does not
                self.hops.append((kind, f, rt.binary_dispatch(kind, dt, tm, tn, tn, tn, tn, f)))
            else:
                self.hops.append((op[1], 0, rt.unary_dispatch(op[1], dt, tm, tn, tn, tn, 0)))
        self.d = [dev(self.A), dev(self.W), dev(self.C)] + [dev(o) for o in self.others] + [dev(o) for o in self.outs]

    def tile_calls(self, t):
        """the invokes of tile t as (kind, args) in program order, on device or host buffers"""
        i, j = divmod(t, self.NB)
        ts = self.tm * self.tn
        calls = [("gemm", (i * self.KB * self.tm * self.tk, j * self.KB * self.tk * self.tn, t * ts))]
        cur, cur_off = "C", t * ts
        for s, op in enumerate(self.ops):
            out, out_off = (("O%d" % s), t * ts) if self.separate else (cur, cur_off)
            calls.append((op, s, cur, cur_off, out, out_off))
            cur, cur_off = out, out_off
        return calls

    def buffers(self, host_side):
        if host_side:
            b = {"A": self.A, "W": self.W, "C": self.C}
            for s in range(len(self.ops)):
                b["R%d" % s], b["O%d" % s] = self.others[s], self.outs[s]
            return b
        b = {"A": self.d[0], "W": self.d[1], "C": self.d[2]}
        n = len(self.ops)
        for s in range(n):
            b["R%d" % s], b["O%d" % s] = self.d[3 + s], self.d[3 + n + s]
        return b

    def run_tile(self, t, b=None, oracle=False):
        b = b or self.buffers(oracle)
        rt, dt = self.rt, self.dt
        for c in self.tile_calls(t):
            if c[0] == "gemm":
                oa, ow, oc = c[1]
                if oracle:
                    orc.brgemm(*self.gdisp, b["A"], oa, b["W"], ow, b["C"], oc, self.KB)
                else:
                    rt.brgemm(dt, self.hg, b["A"], oa, b["W"], ow, b["C"], oc, self.KB)
                continue
            op, s, cur, cur_off, out, out_off = c
            kind, f, h = self.hops[s]
            r_off = cur_off  # the other operand: tile t of R (a broadcast reads its first row / column / element)
            if op[0] == "binary":
                lhs, lo, rhs, ro = (cur, cur_off, "R%d" % s, r_off) if op[3] == 0 else ("R%d" % s, r_off, cur, cur_off)
                if oracle:
                    orc.binary(kind, dt, self.tm, self.tn, self.tn, self.tn, self.tn, f, b[lhs], lo, b[rhs], ro, b[out], out_off)
                else:
                    rt.binary(dt, h, b[lhs], lo, b[rhs], ro, b[out], out_off)
            else:
                if oracle:
                    orc.unary(kind, dt, self.tm, self.tn, self.tn, self.tn, 0, b[cur], cur_off, b[out], out_off)
                else:
                    rt.unary(dt, h, b[cur], cur_off, b[out], out_off)

    def iteration(self):
        b = self.buffers(False)
        for t in range(self.MB * self.NB):
            self.run_tile(t, b)

    def results(self):
        self.rt.synchronize()
        return [host(x, self.dt) for x in [self.d[2]] + self.d[3 + len(self.ops):]]

    def oracle(self):
        b = self.buffers(True)
        b = {k: v.copy() for k, v in b.items()}
        for t in range(self.MB * self.NB):
            self.run_tile(t, b, oracle=True)
        return [b["C"]] + [b["O%d" % s] for s in range(len(self.ops))]


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, ref, what):
    for g, r in zip(got, ref):
        g, r = bits(g), bits(r)
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, "%s: %d elements differ, first at %d: %s vs %s" % (what, bad.size, bad[0], g[bad[0]], r[bad[0]])


def oracle_bits(got, ref, what):
    """against the oracle: finite results bit for bit, non-finite ones by kind (NaN payloads are not pinned)"""
    for g, r in zip(got, ref):
        ed.check_bits(g, r, F32 if g.dtype == np.float32 else BF16, what, special=True)


def run(rt, fold, iters, **kw):
    """iters iterations of a fresh layer with the fold on / off; (results, tile-queue launches and fold stats over all but the first 2)"""
    prev = rt.set_fold_epilogue(fold)
    try:
        L = Layer(rt, **kw)
        for _ in range(min(2, iters)):
            L.iteration()
        rt.synchronize()
        q0, f0 = rt.tile_queue_stats(), rt.fold_epilogue_stats()
        for _ in range(iters - 2):
            L.iteration()
        res = L.results()
        q1, f1 = rt.tile_queue_stats(), rt.fold_epilogue_stats()
        return L, res, q1[0] - q0[0], [b - a for a, b in zip(f0, f1)]
    finally:
        rt.set_fold_epilogue(prev)


LAYERS = {  # M, N, K, tm, tn, tk
    "f32_32x32": (F32, 256, 1024, 256, 32, 32, 32),
    "bf16_64x64": (BF16, 256, 1024, 256, 64, 64, 64),
}


@pytest.mark.parametrize("case,ops", [
    ("f32_32x32", [("binary", ADD, "col", 1)]),     # brgemm + binary add bcast_col_in0 (the bias in position 0)
    ("bf16_64x64", [("binary", ADD, "col", 1)]),
    ("f32_32x32", [("binary", ADD, "col", 0), ("unary", U_RELU)]),  # bias in position 1, then relu
])
def test_timing_loop_is_one_group_per_iteration(rt, case, ops):
    """10 iterations of a layer of tile invokes with a per-tile epilogue: after warm-up every iteration is ONE queued group (the GEMM
    launch + its epilogue program), not one launch per invoke; every post-op of an iteration is folded; bits equal the fold off"""
    dt, M, N, K, tm, tn, tk = LAYERS[case]
    kw = dict(dt=dt, M=M, N=N, K=K, tm=tm, tn=tn, tk=tk, ops=ops, seed=1)
    tiles = (M // tm) * (N // tn)
    _, on, launches, fe = run(rt, True, 10, **kw)
    family = rt.last_grouped_kernel()
    assert "brgemm_grouped" not in family, family  # (the tuned family of these tiles - loader-wave / small32 -, not the generic kernel)
    assert launches <= 8, (launches, fe)
    assert fe[0] >= 8 * tiles * len(ops) and fe[1] <= 8, fe
    L, off, launches_off, _ = run(rt, False, 10, **kw)
    assert launches_off >= 8 * tiles, launches_off
    same_bits(on, off, "fold on vs off")
    ref = L.oracle()
    oracle_bits(on, ref, "fold on vs the oracle (one pass: beta = 0, a fresh result every iteration)")


OPS = [ADD, SUB, MUL, DIV]


@pytest.mark.parametrize("case", ["f32_32x32", "bf16_64x64", "f32_generic"])
def test_bit_identity_matrix(rt, case):
    """{add, sub, mul, div} x {none, row, col, scalar} x {tile as in0, as in1} x {in place, separate output}, special values in the other
    operand (inf, NaN, -0, subnormals, zeros: x / 0): fold on = fold off = the oracle, bit for bit"""
    forced = None
    if case == "f32_generic":
        dt, M, N, K, tm, tn, tk = F32, 128, 128, 64, 32, 32, 32
        forced = 8
    else:
        dt, M, N, K, tm, tn, tk = LAYERS[case]
        M, N = 128, 4 * tn
    if forced is not None:
        rt.force_variant(forced)
    try:
        families = set()
        for op in OPS:
            for bc in BCAST:
                for pos in (0, 1):
                    for sep in (False, True):
                        kw = dict(dt=dt, M=M, N=N, K=K, tm=tm, tn=tn, tk=tk, ops=[("binary", op, bc, pos)], separate=sep, seed=op * 10 + pos,
                                  special=True)
                        L, on, _, fe = run(rt, True, 3, **kw)
                        families.add(rt.last_grouped_kernel())
                        assert fe[0] > 0, (op, bc, pos, sep, fe)
                        _, off, _, _ = run(rt, False, 3, **kw)
                        what = "op %d bcast %s pos %d separate %s" % (op, bc, pos, sep)
                        same_bits(on, off, what + ": on vs off")
                        oracle_bits(on, L.oracle(), what + ": on vs oracle")
        if forced is not None:
            assert any("brgemm_grouped" in f for f in families), families
    finally:
        if forced is not None:
            rt.force_variant(-1)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("ops", [
    [("unary", U_RELU)], [("unary", U_IDENTITY)], [("unary", U_ZERO)],
    [("binary", ADD, "col", 1), ("unary", U_RELU)], [("binary", MUL, "scalar", 0), ("binary", SUB, "none", 1)],
    [("binary", DIV, "row", 0), ("unary", U_IDENTITY)],
], ids=["relu", "identity", "zero", "bias_relu", "scale_residual", "div_identity"])
@pytest.mark.parametrize("sep", [False, True], ids=["in_place", "separate"])
def test_unary_and_two_stage_chains(rt, dt, ops, sep):
    if sep and ops[0] == ("unary", U_ZERO):
        ops = [("unary", U_ZERO), ("unary", U_RELU)]  # (a zero into another buffer reads nothing of the tile: in place, then a stage that is not)
        sep = False
    tm = 32 if dt == F32 else 64
    kw = dict(dt=dt, M=128, N=4 * tm, K=2 * tm, tm=tm, tn=tm, tk=tm, ops=ops, separate=sep, seed=5, special=True)
    L, on, _, fe = run(rt, True, 4, **kw)
    assert fe[0] > 0, fe
    _, off, _, _ = run(rt, False, 4, **kw)
    same_bits(on, off, "on vs off")
    oracle_bits(on, L.oracle(), "on vs oracle")


def test_declines_stay_correct(rt):
    """ineligible element-wise invokes on a queued GEMM group flush it as before (the ineligible counter moves) and the results are
    the unfolded ones: a partial-tile input, a second operand a queued item writes, an output over another item's operand, a third post-op"""
    dt, tm = F32, 32
    rng = np.random.default_rng(9)
    nt, ts = 16, tm * tm
    A, W = exact(rng, nt * ts, dt), exact(rng, ts * 2, dt)
    h = rt.brgemm_dispatch(dt, tm, tm, tm, tm, tm, tm, ts, ts, 4)
    h_half = rt.binary_dispatch(ADD, dt, tm // 2, tm, tm, tm, tm, 0)  # half a tile: not the item's footprint
    h_add = rt.binary_dispatch(ADD, dt, tm, tm, tm, tm, tm, 0)
    h_relu = rt.unary_dispatch(U_RELU, dt, tm, tm, tm, tm, 0)

    def program(fold):
        prev = rt.set_fold_epilogue(fold)
        C = dev(np.zeros(nt * ts, np.float32))
        O = dev(np.zeros(nt * ts, np.float32))
        dA, dW = dev(A), dev(W)
        f0 = rt.fold_epilogue_stats()
        for t in range(nt):
            rt.brgemm(dt, h, dA, t * ts, dW, 0, C, t * ts, 1)
        rt.binary(dt, h_half, C, 0, dA, 0, C, 0)                       # partial tile
        for t in range(nt):
            rt.brgemm(dt, h, dA, t * ts, dW, 0, C, t * ts, 1)
        rt.binary(dt, h_add, C, 1 * ts, C, 2 * ts, O, 1 * ts)         # other operand written by a queued item
        for t in range(nt):
            rt.brgemm(dt, h, dA, t * ts, dW, 0, C, t * ts, 1)
        rt.binary(dt, h_add, C, 3 * ts, dA, 0, dA, ts)                # output over another item's operand (A of tile 1)
        for t in range(nt):
            rt.brgemm(dt, h, dA, t * ts, dW, 0, C, t * ts, 1)
        for t in range(nt):                                           # three stages on tile 0: the third flushes
            rt.unary(dt, h_relu, C, t * ts, C, t * ts)
            if t == 0:
                rt.unary(dt, h_relu, C, 0, C, 0)
                rt.unary(dt, h_relu, C, 0, C, 0)
        rt.synchronize()
        f1 = rt.fold_epilogue_stats()
        rt.set_fold_epilogue(prev)
        return [host(C, dt), host(O, dt), host(dA, dt)], [b - a for a, b in zip(f0, f1)]

    on, fe = program(True)
    off, _ = program(False)
    same_bits(on, off, "declines")
    assert fe[2] >= 4, fe


def test_sync_mode_post_ops_are_not_folded():
    rt = pkg.get_runtime()
    prev_async, prev_q = rt.set_async(False), rt.set_tile_queue(1)
    try:
        f0 = rt.fold_epilogue_stats()
        L = Layer(rt, F32, 64, 64, 32, 32, 32, 32, [("binary", ADD, "col", 1)], seed=3)
        L.iteration()
        res = L.results()
        oracle_bits(res, L.oracle(), "sync mode")
        assert rt.fold_epilogue_stats()[0] == f0[0]
    finally:
        rt.set_tile_queue(prev_q)
        rt.set_async(prev_async)


def test_several_callers_interleave_their_tiles(rt):
    """four threads (ctypes releases the GIL) each issue gemm, add, relu over their own tiles, 20 iterations: the bits of one caller,
    and the launch count per iteration stays bounded"""
    dt, M, N, K, tm, tn, tk = LAYERS["f32_32x32"]
    ops = [("binary", ADD, "col", 1), ("unary", U_RELU)]
    kw = dict(dt=dt, M=M, N=N, K=K, tm=tm, tn=tn, tk=tk, ops=ops, seed=11)
    _, single, _, _ = run(rt, True, 4, **kw)
    L = Layer(rt, **kw)
    b = L.buffers(False)
    nt = L.MB * L.NB
    iters, T = 20, 4
    bar = threading.Barrier(T)

    marks = {}

    def worker_marked(w):
        for it in range(iters):
            for t in range(w, nt, T):
                L.run_tile(t, b)
            bar.wait()
            if w == 0:
                rt.flush()
                if it == 9:  # the steady state: the last 10 iterations
                    marks["q"], marks["f"] = rt.tile_queue_stats(), rt.fold_epilogue_stats()
            bar.wait()

    ths = [threading.Thread(target=worker_marked, args=(w,)) for w in range(T)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    multi = L.results()
    launches = rt.tile_queue_stats()[0] - marks["q"][0]
    folded = rt.fold_epilogue_stats()[0] - marks["f"][0]
    same_bits(multi, single, "four callers vs one")
    assert launches <= 10, launches  # one group per iteration once the group is replayed
    assert folded == 10 * nt * len(ops), folded


STRICT_SCRIPT = r"""
import importlib, sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_fold_epilogue_gpu as T
rt = T.pkg.get_runtime(); rt.set_async(True); rt.set_tile_queue(1)
dt, M, N, K, tm, tn, tk = T.LAYERS["f32_32x32"]
L, res, launches, fe = T.run(rt, True, 6, dt=dt, M=M, N=N, K=K, tm=tm, tn=tn, tk=tk, ops=[("binary", T.ADD, "col", 1), ("unary", T.U_RELU)], seed=4)
np.save(sys.argv[2], np.concatenate([r.view(np.uint32) for r in res]))
print("LAUNCHES", launches, rt.get_strict())
"""


def test_strict_mode_same_bits_same_launches(tmp_path):
    outs = {}
    for strict in ("0", "1"):
        env = dict(os.environ, TPP_HIP_STRICT=strict)
        f = str(tmp_path / ("s%s.npy" % strict))
        r = subprocess.run([sys.executable, "-c", STRICT_SCRIPT, ROOT, f], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [x for x in r.stdout.splitlines() if x.startswith("LAUNCHES")][0].split()
        assert line[2] == strict
        outs[strict] = (np.load(f), int(line[1]))
    assert (outs["0"][0] == outs["1"][0]).all()
    assert outs["0"][1] == outs["1"][1] <= 4, outs


BRHINT_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_fold_epilogue_gpu as T
rt = T.pkg.get_runtime(); rt.set_async(True); rt.set_tile_queue(1)
M, N, K, tm = 256, 1024, 256, 32
MB, NB, KB = M // tm, N // tm, K // tm
ts = tm * tm
rng = np.random.default_rng(21)
A = rng.uniform(-1, 1, M * K).astype(np.float32)    # NOT exact: the summation order shows in the bits
W = rng.uniform(-1, 1, K * N).astype(np.float32)
R = rng.uniform(-1, 1, M * N).astype(np.float32)
h = rt.brgemm_dispatch(T.F32, tm, tm, tm, tm, tm, tm, ts, ts, 4)
ha = rt.binary_dispatch(T.ADD, T.F32, tm, tm, tm, tm, tm, 0)
out = {}
for fold in (1, 0):
    rt.set_fold_epilogue(fold)
    OC = torch.zeros(2 * M * N, dtype=torch.float32, device="cuda")  # ONE allocation: the separate output O below C
    O, C = OC[: M * N], OC[M * N:]
    dA, dW, dR = T.dev(A), T.dev(W), T.dev(R)
    fams = []
    for it in range(6):
        for i in range(MB):
            for j in range(NB):
                t = i * NB + j
                rt.brgemm(T.F32, h, dA, i * KB * ts, dW, j * KB * ts, C, t * ts, KB)
                rt.binary(T.F32, ha, C, t * ts, dR, t * ts, O, t * ts)
        rt.synchronize()
        fams.append(rt.last_grouped_kernel())
    out[fold] = (OC.cpu().numpy().view(np.uint32).copy(), fams)
print("FAMILIES", out[1][1])
assert len(set(out[1][1])) == 1, out[1][1]  # the recording pass and the replays run one family
if rt.get_strict():
    assert (out[1][0] == out[0][0]).all(), int((out[1][0] != out[0][0]).sum())
print("OK")
"""


@pytest.mark.parametrize("strict", ["0", "1"])
def test_separate_output_below_c_keeps_the_family_and_strict_bits(strict):
    """a folded group whose separate output lies below every GEMM output (its post-ops sort first in the recorded group): the replays
    run the family of the recording pass, and in strict mode the bits on non-exact data equal the fold off"""
    env = dict(os.environ, TPP_HIP_STRICT=strict)
    r = subprocess.run([sys.executable, "-c", BRHINT_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]


def test_flat_layout_with_strides_and_poisoned_gaps(rt):
    """tiles of a FLAT row-major C (ldc > the tile width), a residual with its own ld, a separate output with another ld: gaps between
    the tiles' rows and guard bands around every buffer are poisoned and must come back untouched; fold on = fold off = the oracle"""
    dt, M, N, K, tm = F32, 128, 256, 64, 32
    ldc, ldr, ldo, guard = N + 8, N + 16, N + 24, 64
    rng = np.random.default_rng(31)
    A = exact(rng, M * K, dt)
    W = exact(rng, K * N, dt)
    h = rt.gemm_dispatch(dt, tm, tm, K, K, N, ldc, 4)
    ha = rt.binary_dispatch(SUB, dt, tm, tm, ldr, ldc, ldo, 0)   # residual - tile (the tile in position 1)
    hr = rt.unary_dispatch(U_RELU, dt, tm, tm, ldo, ldo, 0)
    poison = ed.poison_fill(guard + M * max(ldc, ldr, ldo) + guard, dt)

    def program(fold):
        prev = rt.set_fold_epilogue(fold)
        Cb, Ob = poison.copy(), poison.copy()
        Rb = poison.copy()
        live = (np.arange(M * ldr) % ldr) < N
        Rb[guard: guard + M * ldr] = np.where(live, exact(np.random.default_rng(32), M * ldr, dt), Rb[guard: guard + M * ldr])
        dC, dO, dR, dA, dW = dev(Cb), dev(Ob), dev(Rb), dev(A), dev(W)
        for _ in range(3):
            for i in range(M // tm):
                for j in range(N // tm):
                    rt.gemm(dt, h, dA, i * tm * K, dW, j * tm, dC, guard + i * tm * ldc + j * tm)
                    rt.binary(dt, ha, dR, guard + i * tm * ldr + j * tm, dC, guard + i * tm * ldc + j * tm, dO, guard + i * tm * ldo + j * tm)
                    rt.unary(dt, hr, dO, guard + i * tm * ldo + j * tm, dO, guard + i * tm * ldo + j * tm)
        rt.synchronize()
        rt.set_fold_epilogue(prev)
        return [host(dC, dt), host(dO, dt)], Rb

    on, Rb = program(True)
    off, _ = program(False)
    same_bits(on, off, "flat layout: on vs off")
    C, O = poison.copy(), poison.copy()
    for i in range(M // tm):
        for j in range(N // tm):
            co, ro, oo = guard + i * tm * ldc + j * tm, guard + i * tm * ldr + j * tm, guard + i * tm * ldo + j * tm
            orc.gemm(dt, tm, tm, K, K, N, ldc, 4, A, i * tm * K, W, j * tm, C, co)
            orc.binary(SUB, dt, tm, tm, ldr, ldc, ldo, 0, Rb, ro, C, co, O, oo)
            orc.unary(U_RELU, dt, tm, tm, ldo, ldo, 0, O, oo, O, oo)
    same_bits(on, [C, O], "flat layout: on vs the oracle, gaps and guard bands included")
