"""Mode 2 of xsmm_hip_set_fold_transpose (include/tpp_xsmm_abi.h): folded transposes read with 16-byte loads, and a transposed A operand
folded like B. Asynchronous mode, tile queue on, device buffers; every case is ONE temporary and eight (transpose, gemm) tile pairs in
one queue group, ended by a synchronisation point.

Per case: the kernel the group ran on (16-byte instance or element instance of its form); for B the bits of mode 1 over the whole C
buffer; on the exact inputs of tests/exact_data.py the oracle's bits; the same values at an aligned and at a misaligned address give the
same bits (16-byte path against element path); uniform data within check_close of the oracle run in program order; NaN / infinity
patterns in every guard band and row gap (source, the other operand, C, around the temporary) reach no output and stay as they are;
the temporary holds the last transpose after the synchronisation point; the fold counters move by (8, 7, 1).
Then the life cycle of an A fold: what must not fold, and what launches the remembered transpose."""
import importlib
import json
import os
import subprocess
import sys
import threading
from collections import namedtuple

import numpy as np
import pytest

import exact_data as ed
from oracle import pyoracle as orc
from test_parity_gpu import BF16, F32, check_close, dev, host

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSPOSE, IDENTITY, BETA0 = 29, 1, 4
NT, G = 8, 64  # tile pairs per case; guard band (floats) in front of and behind every buffer's tiles
BT_V4, BT_EL = "brgemm_grouped<f32,v4>, B read transposed", "brgemm_grouped<f32>, B read transposed"
AT_V4, AT_EL = "brgemm_grouped<f32,v4>, A read transposed", "brgemm_grouped<f32>, A read transposed"

# op: the operand the temporary feeds. transpose [tm, tn, ldi, tm]: source tile tm x tn with leading dimension ldi, temporary tn x tm.
# B: gemm [m, n = tm, k = tn, lda = ld_other, ldb = tm, ldc];  A: gemm [m = tn, n, k = tm, lda = tm, ldb = ld_other, ldc].
# shift: floats the source (src) or the other operand (oth) is moved off 16-byte alignment IN THE CASE ITSELF; vec: the 16-byte
# instance is reached (then the same values one float further on must take the element path and give the same bits)
Case = namedtuple("Case", "id op tm tn ldi m n k ld_other ldc flags shift_src shift_oth vec")
CASES = [
    # B, 16-byte path reached
    Case("B-32x32x64-reference-tile", "B", 32, 64, 512, 32, 32, 64, 512, 32, BETA0, 0, 0, True),   # two chunks
    Case("B-64x48x64-ragged-column-tile", "B", 48, 64, 80, 64, 48, 64, 72, 56, 0, 0, 0, True),
    Case("B-40x34x36-ragged", "B", 34, 36, 52, 40, 34, 36, 44, 38, 0, 0, 0, True),  # n % 4 != 0, ragged m, k % 4 == 0 but % 32 != 0, ld % 32 != 0
    Case("B-32x32x4-one-partial-chunk", "B", 32, 4, 8, 32, 32, 4, 12, 36, 0, 0, 0, True),
    # B, element path
    Case("B-source-misaligned", "B", 32, 64, 512, 32, 32, 64, 512, 32, BETA0, 1, 0, False),
    Case("B-source-ld50", "B", 34, 36, 50, 40, 34, 36, 44, 38, 0, 0, 0, False),
    Case("B-k30", "B", 32, 30, 512, 32, 32, 30, 40, 36, 0, 0, 0, False),
    Case("B-A-misaligned", "B", 32, 64, 512, 32, 32, 64, 512, 32, BETA0, 0, 1, False),
    # A, 16-byte path reached
    Case("A-32x64x32-base", "A", 32, 32, 512, 32, 64, 32, 512, 512, BETA0, 0, 0, True),
    Case("A-36x48x40-ragged-m-and-k", "A", 40, 36, 72, 36, 48, 40, 56, 52, 0, 0, 0, True),
    Case("A-64x32x64-limits", "A", 64, 64, 64, 64, 32, 64, 36, 40, 0, 0, 0, True),
    # A, element path
    Case("A-m34", "A", 32, 34, 72, 34, 32, 32, 36, 40, 0, 0, 0, False),
    Case("A-source-misaligned", "A", 32, 32, 512, 32, 64, 32, 512, 512, BETA0, 1, 0, False),
]


@pytest.fixture(scope="module")
def rt():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


class Switches:
    """asynchronous mode, the tile queue and the fold mode for the duration of a block; everything restored on the way out"""

    def __init__(self, rt, fold):
        self.rt, self.fold = rt, fold

    def __enter__(self):
        self.old = (self.rt.set_async(True), self.rt.set_tile_queue(1))
        self.old_fold = self.rt.set_fold_transpose(self.fold)
        return self

    def __exit__(self, *exc):
        try:
            self.rt.synchronize()
        finally:
            self.rt.set_fold_transpose(self.old_fold if self.old_fold == 2 else bool(self.old_fold))
            self.rt.set_tile_queue(self.old[1])
            self.rt.set_async(self.old[0])


def geometry(c):
    """rows / live columns / leading dimension of the other operand, and the handles' leading dimensions"""
    if c.op == "B":
        assert (c.n, c.k) == (c.tm, c.tn)
        return dict(o_rows=c.m, o_cols=c.k, lda=c.ld_other, ldb=c.tm)
    assert (c.m, c.k) == (c.tn, c.tm)
    return dict(o_rows=c.k, o_cols=c.n, lda=c.tm, ldb=c.ld_other)


def values(c, kind):
    """the live values of a case: source tiles [NT][tm][tn], other-operand tiles, C tiles. exact: integers on a power-of-two grid whose
    every partial sum is an f32 number (exact_data.py); uniform: [-1, 1)"""
    g = geometry(c)
    rng = np.random.default_rng(sum(map(ord, c.id + kind)))
    shapes = ((NT, c.tm, c.tn), (NT, g["o_rows"], g["o_cols"]), (NT, c.m, c.n))
    if kind == "exact":
        ra, rb, rc = ed.exact_ranges(F32, c.k)
        r_src, r_oth = (rb, ra) if c.op == "B" else (ra, rb)
        e_src, e_oth = -3, 2
        return [ed.exact_fill(rng, int(np.prod(s)), F32, R, e).reshape(s) for s, R, e in zip(shapes, (r_src, r_oth, rc), (e_src, e_oth, e_src + e_oth))]
    return [rng.uniform(-1, 1, s).astype(np.float32) for s in shapes]


def place(c, vals, shift_src, shift_oth):
    """the buffers of a case: poison everywhere (guard bands, row gaps, the temporary and its surroundings), the live values at their
    places. Returns the buffers, the tile offsets and C's live mask"""
    g = geometry(c)
    src_v, oth_v, c_v = vals
    n_src, n_oth, n_c = G + NT * c.tm * c.ldi + 4 + G, G + NT * g["o_rows"] * c.ld_other + 4 + G, G + NT * c.m * c.ldc + G
    buf = {"S": ed.poison_fill(n_src, F32), "O": ed.poison_fill(n_oth, F32), "C": ed.poison_fill(n_c, F32), "T": ed.poison_fill(G + c.tn * c.tm + G, F32)}
    off = {"S": [G + shift_src + t * c.tm * c.ldi for t in range(NT)], "O": [G + shift_oth + t * g["o_rows"] * c.ld_other for t in range(NT)],
           "C": [G + t * c.m * c.ldc for t in range(NT)], "T": G}
    live_c = np.zeros(n_c, bool)
    for t in range(NT):
        for name, v, ld in (("S", src_v, c.ldi), ("O", oth_v, c.ld_other), ("C", c_v, c.ldc)):
            rows, cols = v.shape[1:]
            idx = off[name][t] + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
            buf[name][idx] = v[t]
            if name == "C":
                live_c[idx] = True
    return buf, off, live_c


def operands(c, off, t):
    """(A buffer, A offset, B buffer, B offset) of tile t"""
    return ("O", off["O"][t], "T", off["T"]) if c.op == "B" else ("T", off["T"], "O", off["O"][t])


_oracle = {}


def oracle(c, kind):
    """the program in order on the CPU, once per case and kind of data (the results do not depend on where the inputs are placed)"""
    if (c.id, kind) not in _oracle:
        g = geometry(c)
        buf, off, live_c = place(c, values(c, kind), 0, 0)
        for t in range(NT):
            orc.unary(TRANSPOSE, F32, c.tm, c.tn, c.ldi, c.tm, 0, buf["S"], off["S"][t], buf["T"], off["T"])
            a, ao, b, bo = operands(c, off, t)
            orc.gemm(F32, c.m, c.n, c.k, g["lda"], g["ldb"], c.ldc, c.flags, buf[a], ao, buf[b], bo, buf["C"], off["C"][t])
        for v in buf.values():
            v.setflags(write=False)
        _oracle[(c.id, kind)] = (buf, live_c)
    return _oracle[(c.id, kind)]


def run(rt, c, kind, fold, shift_src, shift_oth):
    """the case on the GPU under fold mode `fold`: the buffers afterwards, the inputs as placed, the group's kernel, the counters' moves"""
    g = geometry(c)
    buf, off, _ = place(c, values(c, kind), shift_src, shift_oth)
    d = {k: dev(v) for k, v in buf.items()}
    ht = rt.unary_dispatch(TRANSPOSE, F32, c.tm, c.tn, c.ldi, c.tm, 0)
    hg = rt.gemm_dispatch(F32, c.m, c.n, c.k, g["lda"], g["ldb"], c.ldc, c.flags)
    with Switches(rt, fold):
        f0 = rt.fold_transpose_stats()
        for t in range(NT):
            rt.unary(F32, ht, d["S"], off["S"][t], d["T"], off["T"])
            a, ao, b, bo = operands(c, off, t)
            rt.gemm(F32, hg, d[a], ao, d[b], bo, d["C"], off["C"][t])
        rt.synchronize()
        f1 = rt.fold_transpose_stats()
        name = rt.last_grouped_kernel()
    return {k: host(v, buf[k]) for k, v in d.items()}, buf, name, tuple(x - y for x, y in zip(f1, f0))


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def names_of(c):
    """(kernel of the case as given, kernel of the same values with the source one float further on)"""
    v4, el = (BT_V4, BT_EL) if c.op == "B" else (AT_V4, AT_EL)
    return (v4 if c.vec else el), el


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_exact_inputs_kernel_bits_poison_and_counters(rt, c):
    want, want_off = names_of(c)
    ref, live_c = oracle(c, "exact")
    got, placed, name, moved = run(rt, c, "exact", 2, c.shift_src, c.shift_oth)
    print("%s: mode 2 ran on [%s], counters moved by %s" % (c.id, name, moved))
    assert moved == (NT, NT - 1, 1), "folded / dropped / launched: %s" % (moved,)
    assert name == want, name
    # the oracle's bits in every live element of C - and, comparing the whole buffers, every poisoned gap and guard band as it was
    ed.check_bits(got["C"][live_c], ref["C"][live_c], F32, c.id + ": C")
    assert same_bits(got["C"], ref["C"]), "C's row gaps or guard bands changed"
    assert np.isfinite(got["C"][live_c]).all()
    assert same_bits(got["T"], ref["T"]), "the temporary holds the last transpose (and its guard bands their poison) after the synchronisation point"
    for k in ("S", "O"):
        assert same_bits(got[k], placed[k]), "an input buffer changed: " + k
    # the same values one float off (or, for a case that is misaligned itself, back on) 16-byte alignment: the other instance, the same bits
    other = dict(shift_src=0, shift_oth=0) if (c.shift_src or c.shift_oth) else dict(shift_src=1, shift_oth=0)
    got2, _, name2, moved2 = run(rt, c, "exact", 2, **other)
    print("%s: moved to shifts %s: [%s]" % (c.id, other, name2))
    assert moved2 == (NT, NT - 1, 1), moved2
    if c.vec:
        assert name2 == want_off, name2
    elif c.shift_src or c.shift_oth:
        assert name2 == (BT_V4 if c.op == "B" else AT_V4), name2  # (the misaligned cases are 16-byte cases but for their address)
    else:
        assert name2 == want_off, name2
    assert same_bits(got2["C"], got["C"]), "16-byte path and element path differ in bits"
    assert same_bits(got2["T"], got["T"])
    if c.op == "B":  # mode 1 on the same buffers: the whole C buffer, gaps included
        got1, _, name1, moved1 = run(rt, c, "exact", 1, c.shift_src, c.shift_oth)
        assert name1 == BT_EL, name1
        assert moved1 == (NT, NT - 1, 1), moved1
        assert same_bits(got1["C"], got["C"]), "mode 2 differs from mode 1 in bits"
        assert same_bits(got1["T"], got["T"])


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_uniform_data_close_to_the_oracle_in_program_order(rt, c):
    ref, live_c = oracle(c, "uniform")
    got, placed, name, moved = run(rt, c, "uniform", 2, c.shift_src, c.shift_oth)
    assert moved == (NT, NT - 1, 1), moved
    assert name == names_of(c)[0], name
    check_close(got["C"][live_c], ref["C"][live_c], F32, "%s [%s]" % (c.id, name), K=c.k)
    assert same_bits(got["C"][~live_c], ref["C"][~live_c]), "C's row gaps or guard bands changed"
    assert same_bits(got["T"], ref["T"])
    if c.op == "B":
        got1, _, name1, _ = run(rt, c, "uniform", 1, c.shift_src, c.shift_oth)
        assert name1 == BT_EL, name1
        assert same_bits(got1["C"], got["C"]), "mode 2 differs from mode 1 in bits"


# ---- the life cycle of an A fold --------------------------------------------------------------------------------------------------
S, E = 32, 512


def a_program(case):
    """three (transpose, gemm) pairs whose gemm reads the temporary as its A operand. Returns (dtype, the initial buffers, the call
    list) - calls: ("t", src offset) / ("g", A buffer, A offset, B buffer, B offset, C buffer, C offset) -, the two dispatch tuples
    and the batch count"""
    rng = np.random.default_rng(41)
    dt = BF16 if case == "bf16" else F32
    tn = 96 if case == "m96" else S                  # the gemm's m
    lda = 40 if case == "lda_not_ldo" else S
    n = S if case == "both_temporary" else 64
    br = 2 if case == "batch2" else 1

    def data(count):
        v = rng.uniform(-1, 1, count).astype(np.float32)
        return v if dt == F32 else orc.f32_to_bf16(v)

    bufs = {"X": data(4 * S * E), "B": data(4 * S * E), "C": data(4 * 96 * E), "T": data(96 * 40 + 64)}
    cbuf = "X" if case == "c_over_source" else "C"
    bbuf, ldb = ("T", S) if case == "both_temporary" else ("B", E)
    calls = []
    for rep in range(3):
        calls.append(("t", rep * 128))
        calls.append(("g", "T", 0, bbuf, 0 if bbuf == "T" else rep * 64, cbuf, (rep * 128 if cbuf == "X" else 256 + rep * 64)))
    t_desc = (TRANSPOSE, dt, S, tn, E, S, 0)
    g_desc = (dt, tn, n, S, lda, ldb, E, 0, S * ldb, BETA0)
    return dt, bufs, calls, t_desc, g_desc, br


def a_oracle(bufs, calls, t_desc, g_desc, br):
    ref = {k: v.copy() for k, v in bufs.items()}
    for c in calls:
        if c[0] == "t":
            orc.unary(*t_desc, ref["X"], c[1], ref["T"], 0)
        else:
            orc.brgemm(*g_desc, ref[c[1]], c[2], ref[c[3]], c[4], ref[c[5]], c[6], br)
    return ref


NOT_FOLDED = ["both_temporary", "batch2", "lda_not_ldo", "c_over_source", "m96", "bf16", "mode1"]


@pytest.mark.parametrize("case", ["folds"] + NOT_FOLDED)
def test_gemm_reading_the_temporary_as_A_folded_or_not_same_results(rt, case):
    """the gemm behind a remembered transpose whose A operand is the temporary: folded when it may be (the first case), else the
    transpose is launched first - either way the oracle's results on the program as written, in every buffer"""
    dt, bufs, calls, t_desc, g_desc, br = a_program(case)
    ref = a_oracle(bufs, calls, t_desc, g_desc, br)
    d = {k: dev(v) for k, v in bufs.items()}
    ht = rt.unary_dispatch(*t_desc)
    hg = rt.brgemm_dispatch(*g_desc)
    with Switches(rt, 1 if case == "mode1" else 2):
        f0 = rt.fold_transpose_stats()
        for c in calls:
            if c[0] == "t":
                rt.unary(dt, ht, d["X"], c[1], d["T"], 0)
            else:
                rt.brgemm(dt, hg, d[c[1]], c[2], d[c[3]], c[4], d[c[5]], c[6], br)
        rt.synchronize()
        f1 = rt.fold_transpose_stats()
        name = rt.last_grouped_kernel()
    assert f1[0] - f0[0] == (3 if case == "folds" else 0), (case, f0, f1)
    if case == "folds":
        assert name == AT_V4, name
        assert (f1[1] - f0[1], f1[2] - f0[2]) == (2, 1)
    for k in bufs:
        check_close(host(d[k], bufs[k]), ref[k], dt, "%s: buffer %s" % (case, k), K=S)


def test_strict_mode_folds_nothing():
    """strict mode is chosen before the first invoke, so this runs in a process of its own - with the mode from the environment
    (TPP_HIP_FOLD_TRANSPOSE=2: read as a number)"""
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_TILE_QUEUE", "TPP_HIP_ASYNC")}
    env.update(TPP_HIP_STRICT="1", TPP_HIP_FOLD_TRANSPOSE="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "trans_operands_worker.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["mode_from_env"] == 2 and out["strict"] == 1, out
    assert out["folded"] == 0, out
    assert out["max_err"] <= 1e-5 * max(1.0, out["max_ref"]), out


def test_setter_returns_the_previous_mode_and_refuses_other_values(rt):
    first = rt.lib.xsmm_hip_set_fold_transpose(2)
    try:
        assert first in (0, 1, 2)
        assert rt.lib.xsmm_hip_set_fold_transpose(3) == -1 and rt.lib.xsmm_hip_set_fold_transpose(-1) == -1
        assert rt.lib.xsmm_hip_set_fold_transpose(0) == 2, "a refused value changed the mode"
        assert rt.set_fold_transpose(True) == 0 and rt.set_fold_transpose(2) == 1 and rt.set_fold_transpose(False) == 2
        assert rt.set_fold_transpose(3) == -1 and rt.set_fold_transpose(1) == 0, "the wrapper passes integers on: 3 is refused, not read as 1"
    finally:
        rt.lib.xsmm_hip_set_fold_transpose(first)


def _a_fold_setup(rt, seed):
    rng = np.random.default_rng(seed)
    X, Y, Bm = (rng.uniform(-1, 1, S * E).astype(np.float32) for _ in range(3))
    tX = np.ascontiguousarray(X.reshape(S, E)[:, :S].T).reshape(-1)
    tY = np.ascontiguousarray(Y.reshape(S, E)[:, :S].T).reshape(-1)
    ht = rt.unary_dispatch(TRANSPOSE, F32, S, S, E, S, 0)
    hg = rt.gemm_dispatch(F32, S, 64, S, S, E, 64, BETA0)
    hc = rt.unary_dispatch(IDENTITY, F32, S, S, S, S, 0)

    def ref_of(t):
        r = np.zeros(S * 64, np.float32)
        orc.gemm(F32, S, 64, S, S, E, 64, BETA0, t, 0, Bm, 0, r, 0)
        return r
    return X, Y, Bm, tX, tY, ht, hg, hc, ref_of


def test_copy_out_of_the_temporary_behind_a_folded_A_gemm_sees_the_transpose(rt):
    X, Y, Bm, tX, tY, ht, hg, hc, ref_of = _a_fold_setup(rt, 42)
    dX, dB, dT, dC, dO = dev(X), dev(Bm), dev(np.zeros(S * S, np.float32)), dev(np.zeros(S * S, np.float32)), dev(np.zeros(S * 64, np.float32))
    with Switches(rt, 2):
        f0 = rt.fold_transpose_stats()
        rt.unary(F32, ht, dX, 0, dT, 0)
        rt.gemm(F32, hg, dT, 0, dB, 0, dO, 0)
        f1 = rt.fold_transpose_stats()
        assert (f1[0] - f0[0], f1[2] - f0[2]) == (1, 0), "folded, the transpose still remembered"
        rt.unary(F32, hc, dT, 0, dC, 0)  # any other invoke of the thread launches it first
        assert rt.fold_transpose_stats()[2] - f0[2] == 1
        rt.synchronize()
        assert np.array_equal(host(dC, tX), tX)
        check_close(host(dO, tX), ref_of(tX), F32, "the folded gemm", K=S)


def test_second_transpose_replaces_the_record_of_an_A_fold(rt):
    X, Y, Bm, tX, tY, ht, hg, hc, ref_of = _a_fold_setup(rt, 43)
    dX, dY, dB, dT = dev(X), dev(Y), dev(Bm), dev(np.zeros(S * S, np.float32))
    dO, dO2 = dev(np.zeros(S * 64, np.float32)), dev(np.zeros(S * 64, np.float32))
    with Switches(rt, 2):
        f0 = rt.fold_transpose_stats()
        rt.unary(F32, ht, dX, 0, dT, 0)
        rt.gemm(F32, hg, dT, 0, dB, 0, dO, 0)
        rt.unary(F32, ht, dY, 0, dT, 0)  # replaces the remembered one: dead, its reader was served from its source
        rt.gemm(F32, hg, dT, 0, dB, 0, dO2, 0)
        f1 = rt.fold_transpose_stats()
        assert tuple(a - b for a, b in zip(f1, f0)) == (2, 1, 0), (f0, f1)
        assert not host(dT, tX).any(), "nothing launched yet (a stream-ordered copy sees the old bytes)"
        rt.flush()
        assert rt.fold_transpose_stats()[2] - f0[2] == 1
        rt.synchronize()
        assert np.array_equal(host(dT, tY), tY)
        check_close(host(dO, tX), ref_of(tX), F32, "gemm behind the first transpose", K=S)
        check_close(host(dO2, tX), ref_of(tY), F32, "gemm behind the second transpose", K=S)


def test_another_thread_touching_the_destination_launches_an_A_folds_transpose_first(rt):
    X, Y, Bm, tX, tY, ht, hg, hc, ref_of = _a_fold_setup(rt, 44)
    dX, dB, dT, dC, dO = dev(X), dev(Bm), dev(np.zeros(S * S, np.float32)), dev(np.zeros(S * S, np.float32)), dev(np.zeros(S * 64, np.float32))
    dC2 = dev(np.zeros(S * S, np.float32))
    with Switches(rt, 2):
        def worker():
            rt.unary(F32, ht, dX, 0, dT, 0)
            rt.gemm(F32, hg, dT, 0, dB, 0, dO, 0)

        f0 = rt.fold_transpose_stats()
        t = threading.Thread(target=worker)
        t.start()
        t.join()
        f1 = rt.fold_transpose_stats()
        assert (f1[0] - f0[0], f1[2] - f0[2]) == (1, 0), "folded, the transpose still remembered"
        rt.unary(F32, hc, dC, 0, dC2, 0)  # touches neither the destination nor (writing) the source: the record stays
        assert rt.fold_transpose_stats()[2] == f1[2]
        rt.unary(F32, hc, dT, 0, dC, 0)  # reads the destination
        assert rt.fold_transpose_stats()[2] - f0[2] == 1
        rt.synchronize()
        assert np.array_equal(host(dC, tX), tX)
