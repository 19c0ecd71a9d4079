"""The host cache on the GPU (csrc/host_cache.cpp; include/tpp_xsmm_abi.h xsmm_hip_set_host_cache): host pointers, the way an unmodified
tpp-run calls the reference (lib/TPP/Runner/MLIRBench.cpp:207-246), with the operands kept on the device between invokes.
Parity = the plain per-invoke mirror path on the same inputs, bit for bit, plus the oracle / golden fixtures where they exist.
Behind the scenarios: seeded coherence programs over every synchronisation point and mode switch, checked byte for byte against numpy
shadows that the oracle keeps (test_coherence_program_* / test_zz_coherence_coverage), and the size edges of the copy paths around
the 4 MiB staging slot (test_copy_path_size_edges)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import fixture_runner as fr
from abi_backend import AbiBackend
from oracle import pyoracle as orc

pkg = importlib.import_module("tpp-mlir_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 1, 2


@pytest.fixture
def rt_cache():
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    prev = r.set_host_cache(True)
    if prev < 0:
        pytest.skip("this kernel lacks userfaultfd WP_ASYNC / PAGEMAP_SCAN: the host cache stays off")
    yield r
    r.set_async(False)
    r.set_tile_queue(0)
    r.set_host_cache(False)


@pytest.mark.parametrize("path", fr.fixtures(), ids=lambda p: os.path.basename(p)[:-5])
def test_golden_fixture_through_host_pointers_with_the_cache(rt_cache, path):
    """the reference's own FileCheck'd numbers (tests/golden/*.json), host pointers, synchronous invokes - with mirrors that outlive the
    invokes (every fixture runs twice: the second pass finds its operands' pages on the device)"""
    fr.run_fixture(path, AbiBackend("host"))
    fr.run_fixture(path, AbiBackend("host"))


_keep = []


def unaligned(n, dtype, off=192):
    """memref.alloc-style: 64-byte aligned, never page aligned - in a FRESH anonymous mapping: pages the ROCm runtime has never been handed.
    (A buffer that was once the source / destination of a plain hipMemcpy stays in the runtime's pin cache, and the driver write-faults its
    pages again after every later piece of driver activity: the kernel's write tracking then reports the whole buffer written - the host
    cache uploads it again, correct but no faster than the plain path. tools/ubench/wp_vs_hipmemcpy.cpp, profiles/r06_wp_vs_hipmemcpy.txt.
    numpy's allocator re-uses the heap addresses of earlier tests' arrays, which went through exactly such copies.)"""
    import mmap
    nbytes = n * np.dtype(dtype).itemsize
    m = mmap.mmap(-1, nbytes + 8192)
    _keep.append(m)
    return np.frombuffer(m, dtype=np.uint8, count=nbytes, offset=off + 64)[:nbytes].view(dtype)


def test_c2_sync_loop_with_host_edits(rt_cache):
    """BASELINE config 2 (BRGEMM 1024^3 f32, br = 16) through host pointers in the reference's synchronous mode: results visible on
    return, identical to the plain mirror path; the host edits A, B (through a system call) and C between invokes"""
    rt = rt_cache
    m = n = 1024
    k, br = 64, 16
    rng = np.random.default_rng(5)
    A, B, C = unaligned(m * 1024, np.float32), unaligned(1024 * n, np.float32), unaligned(m * n, np.float32)
    A[:] = rng.uniform(-1, 1, A.size)
    B[:] = rng.uniform(-1, 1, B.size)
    C[:] = rng.uniform(-1, 1, C.size)
    h = rt.brgemm_dispatch(F32, m, n, k, 1024, 1024, 1024, 64, 65536, 0)  # accumulating: C is read and written
    hb = rt.brgemm_dispatch(F32, m, n, k, 1024, 1024, 1024, 64, 65536, 4)
    A2, B2, C2 = A.copy(), B.copy(), C.copy()

    def program(rt, A, B, C):
        outs = []
        rt.brgemm(F32, h, A, 0, B, 0, C, 0, br)
        outs.append(C.copy())
        rt.brgemm(F32, h, A, 0, B, 0, C, 0, br)
        A[12345] = 3.0
        rt.brgemm(F32, hb, A, 0, B, 0, C, 0, br)
        outs.append(C.copy())
        B[5000:7000] = 0.0
        C[100:2100] = -1.0
        rt.brgemm(F32, h, A, 0, B, 0, C, 0, br)
        outs.append(C.copy())
        return outs

    s0 = rt.host_cache_stats()
    got = program(rt, A, B, C)
    s1 = rt.host_cache_stats()
    rt.set_host_cache(False)
    want = program(rt, A2, B2, C2)
    rt.set_host_cache(True)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    # 12 MiB of operands, four invokes: the plain path uploads 8-12 MiB per invoke (44 MiB); the cache uploads everything once, the pages
    # edited, and C a second time (the BETA_0 invoke leaves its pure output untracked: the accumulating invoke behind it reads it again)
    up = s1["uploaded_bytes"] - s0["uploaded_bytes"]
    assert 12 * 2 ** 20 <= up <= 16 * 2 ** 20 + 64 * 4096, up


def test_c2_async_loop_runs_at_device_speed_and_writes_back_at_the_sync_point(rt_cache):
    """asynchronous mode (TPP_HIP_ASYNC=1): the timing loop of tpp-run on HOST buffers - no upload after the first invoke, the output
    on the host after perf_stop_timer, equal to the device-pointer result"""
    import torch
    rt = rt_cache
    m = n = 1024
    k, br = 64, 16
    rng = np.random.default_rng(6)
    A, B, C = unaligned(m * 1024, np.float32), unaligned(1024 * n, np.float32), unaligned(m * n, np.float32)
    A[:] = rng.uniform(-1, 1, A.size)
    B[:] = rng.uniform(-1, 1, B.size)
    C[:] = 0
    h = rt.brgemm_dispatch(F32, m, n, k, 1024, 1024, 1024, 64, 65536, 4)
    rt.set_async(True)
    rt.brgemm(F32, h, A, 0, B, 0, C, 0, br)
    rt.synchronize()
    s0 = rt.host_cache_stats()
    t0 = rt.perf_start_timer()
    for _ in range(200):
        rt.brgemm(F32, h, A, 0, B, 0, C, 0, br)
    dt = rt.perf_stop_timer(t0)
    s1 = rt.host_cache_stats()
    # (the edge pages of the run written back at the sync point)
    assert s1["uploaded_bytes"] - s0["uploaded_bytes"] <= 16 * 4096, s1
    assert s1["fast_invokes"] - s0["fast_invokes"] >= 199
    dA, dB = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(B.copy()).cuda()
    dC = torch.zeros(m * n, device="cuda")
    rt.brgemm(F32, h, dA, 0, dB, 0, dC, 0, br)
    rt.synchronize()
    assert np.array_equal(C.view(np.uint32), dC.cpu().numpy().view(np.uint32))
    rt.set_async(False)
    # 200 invokes of a 17-18 us kernel: the plain mirror path needs ~300 us each (PCIe); allow generous head room for a shared box
    assert dt / 200 < 60e-6, dt / 200


@pytest.mark.parametrize("threads", [1, 4])
def test_reference_mlp_as_tile_invokes_on_host_buffers(rt_cache, threads):
    """the reference's headline MLP as the compiler emits it (768 invokes of one 32x32x32 dispatch per iteration) on plain host buffers,
    TPP_HIP_ASYNC=1 TPP_HIP_TILE_QUEUE=1 TPP_HIP_HOST_CACHE=1 - environment variables only, no xsmm_hip_* call in the program
    (tools/tpp_replay --host-buffers): the host's output buffer holds the closed-form result behind the timing loop"""
    exe = os.path.join(ROOT, "tools", "tpp_replay")
    if not os.path.exists(exe):
        pytest.skip("tools/tpp_replay not built")
    env = dict(os.environ, TPP_HIP_ASYNC="1", TPP_HIP_TILE_QUEUE="1", TPP_HIP_HOST_CACHE="1")
    r = subprocess.run([exe, "--host-buffers", "--batch", "256", "--layers", "1024,1024,1024,1024", "--tiles", "32", "--bias", "--relu", "-n", "100",
                        "--threads", str(threads)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "host output buffer checked" in r.stderr, r.stderr[-3000:]


def test_mlp_tiles_host_cache_equals_device_pointers_bitwise(rt_cache):
    """random weights: 3 layers of 32x32x32 tile invokes (packed blocks) on host buffers through the tile queue == the same program on
    device pointers, bit for bit; a weight edited between two synchronisation epochs is seen"""
    import torch
    rt = rt_cache
    M, W, T = 128, 256, 32
    MB, NB, KB = M // T, W // T, W // T
    rng = np.random.default_rng(9)
    acts = [unaligned(M * W, np.float32) for _ in range(4)]
    Ws = [unaligned(W * W, np.float32) for _ in range(3)]
    bs = [unaligned(W, np.float32) for _ in range(3)]
    acts[0][:] = rng.uniform(-1, 1, M * W)
    for w in Ws:
        w[:] = rng.uniform(-1, 1, W * W) / 16
    for b in bs:
        b[:] = rng.uniform(-1, 1, W)
    h = rt.fused_brgemm_dispatch(F32, T, T, T, T, T, T, T * T, T * T, 4, 0, 5, 4, 1)

    def iteration(acts, Ws, bs):
        for l in range(3):
            for i in range(MB):
                for j in range(NB):
                    rt.fused_brgemm(F32, h, acts[l], i * KB * T * T, Ws[l], j * KB * T * T, acts[l + 1], (i * NB + j) * T * T, bs[l], j * T, KB)

    rt.set_async(True)
    rt.set_tile_queue(1)
    for edit in (False, True):
        if edit:
            Ws[1][4321] = 0.5
            acts[0][7] = -0.25
        for _ in range(3):
            iteration(acts, Ws, bs)
        rt.synchronize()
        dacts = [torch.from_numpy(a.copy()).cuda() for a in acts]
        dWs = [torch.from_numpy(w.copy()).cuda() for w in Ws]
        dbs = [torch.from_numpy(b.copy()).cuda() for b in bs]
        iteration(dacts, dWs, dbs)
        rt.synchronize()
        for l in range(1, 4):
            assert np.array_equal(acts[l].view(np.uint32), dacts[l].cpu().numpy().view(np.uint32)), (edit, l)
    st = rt.host_cache_stats()
    assert st["fast_invokes"] > 3 * 3 * MB * NB and st["pages_not_written_back"] == 0, st
    rt.set_tile_queue(0)
    rt.set_async(False)


def test_bf16_vnni_layer_on_host_buffers_matches_the_oracle(rt_cache):
    """bf16 + VNNI-2 fused layer (bias + relu) through host pointers with the cache, against the oracle within one bf16 ulp"""
    rt = rt_cache
    m, n, k, br = 256, 512, 64, 8
    rng = np.random.default_rng(11)
    A = orc.f32_to_bf16(rng.uniform(-1, 1, m * k * br).astype(np.float32))
    Bf = rng.uniform(-1, 1, (k * br, n)).astype(np.float32) / 8
    Bv = orc.f32_to_bf16(np.ascontiguousarray(Bf.reshape(k * br // 2, 2, n).transpose(0, 2, 1)).reshape(-1))
    bias = orc.f32_to_bf16(rng.uniform(-1, 1, n).astype(np.float32))
    C = np.zeros(m * n, np.uint16)
    ref = C.copy()
    args = (BF16, m, n, k, k * br, n, n, k, k * n, 4 | 2048, 0, 5, 4, 1)
    orc.fused_brgemm(*args, A, 0, Bv, 0, ref, 0, bias, 0, br)
    h = rt.fused_brgemm_dispatch(*args)
    for _ in range(2):
        rt.fused_brgemm(BF16, h, A, 0, Bv, 0, C, 0, bias, 0, br)
    d = np.abs(orc.bf16_to_f32(C).astype(np.float64) - orc.bf16_to_f32(ref))
    r = np.abs(orc.bf16_to_f32(ref).astype(np.float64))
    assert (d <= r * 2.0 ** -7 + 1e-5 * max(1.0, r.max())).all()


# ---------------------------------------------------------------- seeded coherence programs
# A program is a seeded random sequence of invokes, host edits, synchronisation points and mode switches over a few small host buffers,
# inside the contract of include/tpp_xsmm_abi.h (asynchronous mode: the host reads outputs and writes operands only directly behind a
# synchronisation point). The expected bytes never come from the runtime: every buffer has a numpy SHADOW that the oracle updates
# invoke by invoke in program order, on exact data (small integers: every sum is an f32 number in any order, tests/exact_data.py), so
# the device's bytes must be the oracle's - every byte of every mapping, padding and guard bytes included, no tolerance.
# tests/hostcache/driver.cpp runs the same kind of program on the CPU against plain loops.
import exact_data as ed  # noqa: E402

SYNC_KINDS = ("synchronize", "perf_stop_timer", "set_async(0)+(1)", "set_stream", "set_host_cache(0)+(1)")
SQ, KB, BR, FM, FN, TS, WIN, WIN_OFF, HWIN, HWIN_OFF = 64, 32, 2, 64, 192, 32, 160, 16, 48, 8
IN_MAX = 16            # a GEMM input holds integers up to this (bf16 inputs: far below 2^8) ...
MAX_ACCUMULATIONS = 6  # ... and an output accumulates at most this often between two re-initialisations:
#                        |C| <= 7 * (64 * 16 * 16 + 3) < 2^17, far below 2^24 - asserted on the model's values before every invoke
S0, S1, S2, S3, FL, WI, VB, H0, H1, HA, HB, HC = range(12)
BUFS = (("S0", np.float32, SQ * SQ), ("S1", np.float32, SQ * SQ), ("S2", np.float32, SQ * SQ), ("S3", np.float32, SQ * SQ),
        ("F", np.float32, FM * FN), ("W", np.float32, FM * FN), ("V", np.float32, FN), ("H0", np.uint16, SQ * SQ), ("H1", np.uint16, SQ * SQ),
        ("HA", np.uint16, SQ * SQ), ("HB", np.uint16, SQ * SQ), ("HC", np.uint16, SQ * SQ))
# name -> (family, dispatch arguments as the runtime and the oracle both take them)
OPS = {}
for _b1 in (0, 1):
    _fl = 0 if _b1 else 4
    OPS["whole%d" % _b1] = ("brgemm", (F32, SQ, SQ, KB, SQ, SQ, SQ, KB, KB * SQ, _fl))
    OPS["fused%d" % _b1] = ("fused", (F32, SQ, SQ, KB, SQ, SQ, SQ, KB, KB * SQ, _fl, 0, 5, 4, 1))
    OPS["tile%d" % _b1] = ("brgemm", (F32, TS, TS, KB, SQ, FN, FN, KB, KB * FN, _fl))
    OPS["hgemm%d" % _b1] = ("brgemm", (BF16, SQ, SQ, KB, SQ, SQ, SQ, KB, KB * SQ, _fl))
OPS.update({
    "relu_sq": ("unary", (5, F32, SQ, SQ, SQ, SQ, 0)), "relu_tile": ("unary", (5, F32, TS, TS, FN, FN, 0)),
    "zero_sq": ("unary", (2, F32, SQ, SQ, SQ, SQ, 0)), "zero_tile": ("unary", (2, F32, TS, TS, FN, FN, 0)),
    "ident_win": ("unary", (1, F32, FM, WIN, FN, FN, 0)),
    "add_sq": ("binary", (1, F32, SQ, SQ, SQ, SQ, SQ, 8)), "add_tile": ("binary", (1, F32, TS, TS, FN, TS, FN, 8)),
    "hrelu": ("unary", (5, BF16, SQ, SQ, SQ, SQ, 0)), "hident_win": ("unary", (1, BF16, SQ, HWIN, SQ, SQ, 0)),
    "hzero_tile": ("unary", (2, BF16, TS, TS, SQ, SQ, 0)),
})
GEMM_KINDS = ("brgemm", "fused_brgemm", "brgemm_tile", "bf16_brgemm")
# what a segment does directly behind a synchronisation point: the host edits an input and the invoke that read it runs again; an invoke
# of the last segment writes its output again behind a host edit of that output; the same with the output read as C of a beta-1 GEMM
HALVES = ("edit-then-invoke", "rewrite-an-output", "edit-an-output-a-beta-1-invoke-reads")
INVOKE_KINDS = ("brgemm", "fused_brgemm", "brgemm_tile", "bf16_brgemm", "relu_inplace", "relu_inplace_tile", "zero", "zero_tile", "identity_window",
                "add_bcast_col", "add_bcast_col_tile", "bf16_relu_inplace", "bf16_identity_window", "bf16_zero_tile")
COH_SEEDS = tuple(range(2000, 2060))  # (the count is a time budget: a program takes ~50 ms on the device, the file a few seconds of a suite of several minutes)
COH = {"pair": {}, "kinds": {}, "programs": 0, "steps": 0, "invokes": 0, "edits": 0, "syncs": 0, "checks": 0, "stats0": None, "stats1": None}


class OracleBackend:
    """the model's side of an invoke: the oracle on the shadow arrays"""

    def run(self, op, operands, br):
        fam, args = OPS[op]
        flat = [x for pair in operands for x in pair]
        if fam == "brgemm":
            orc.brgemm(*args, *flat, br)
        elif fam == "fused":
            orc.fused_brgemm(*args, *flat, br)
        elif fam == "unary":
            orc.unary(*args, *flat)
        else:
            orc.binary(*args, *flat)


class RuntimeBackend:
    """the device's side: the C-ABI on host pointers"""

    def __init__(self, rt):
        self.rt, self.h = rt, {}

    def run(self, op, operands, br):
        fam, args = OPS[op]
        rt = self.rt
        if op not in self.h:
            self.h[op] = {"brgemm": rt.brgemm_dispatch, "fused": rt.fused_brgemm_dispatch, "unary": rt.unary_dispatch, "binary": rt.binary_dispatch}[fam](*args)
        flat = [x for pair in operands for x in pair]
        dt = args[0] if fam in ("brgemm", "fused") else args[1]
        if fam == "brgemm":
            rt.brgemm(dt, self.h[op], *flat, br)
        elif fam == "fused":
            rt.fused_brgemm(dt, self.h[op], *flat, br)
        elif fam == "unary":
            rt.unary(dt, self.h[op], *flat)
        else:
            rt.binary(dt, self.h[op], *flat)


class CohBuf:
    OFF, GUARD = 256, 4096 + 320  # data 64-byte aligned, never page aligned; guard bytes behind it

    def __init__(self, name, dtype, n):
        import mmap
        self.name, self.dtype, self.n = name, dtype, n
        nbytes = n * np.dtype(dtype).itemsize
        self.map_bytes = (self.OFF + nbytes + self.GUARD + 4095) // 4096 * 4096
        self.m = mmap.mmap(-1, self.map_bytes)  # a FRESH anonymous mapping (see unaligned())
        self.raw = np.frombuffer(self.m, dtype=np.uint8)
        self.raw[:] = 0xA5
        self.a = self.raw[self.OFF:self.OFF + nbytes].view(dtype)
        self.sraw = np.full(self.map_bytes, 0xA5, np.uint8)
        self.s = self.sraw[self.OFF:self.OFF + nbytes].view(dtype)
        self.dt = F32 if dtype == np.float32 else BF16

    def write(self, lo, values):
        """the host writes elements [lo, lo + len) - and the model with it"""
        v = ed.store(np.asarray(values, np.float32), self.dt)
        self.a[lo:lo + v.size] = v
        self.s[lo:lo + v.size] = v

    def model(self, off, rows, cols, ld):
        idx = off + (np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).reshape(-1)
        return ed.as_f32(self.s[idx]).astype(np.float64)


def footprint_out(v):
    kind, a, b, c, ti, tj, beta1 = v
    if kind in ("brgemm", "fused_brgemm", "bf16_brgemm", "relu_inplace", "zero", "add_bcast_col", "bf16_relu_inplace"):
        return c, 0, SQ, SQ, SQ
    if kind in ("brgemm_tile", "relu_inplace_tile", "zero_tile", "add_bcast_col_tile"):
        return c, ti * TS * FN + tj * TS, TS, TS, FN
    if kind == "identity_window":
        return c, WIN_OFF, FM, WIN, FN
    if kind == "bf16_identity_window":
        return c, HWIN_OFF, SQ, HWIN, SQ
    return c, ti * TS * SQ + tj * TS, TS, TS, SQ  # bf16_zero_tile


def footprint_in(v):
    """one input worth editing (None: the op reads nothing)"""
    kind, a, b, c, ti, tj, beta1 = v
    if kind in ("brgemm", "fused_brgemm", "bf16_brgemm", "add_bcast_col"):
        return a, 0, SQ, SQ, SQ
    if kind == "brgemm_tile":
        return a, ti * TS * SQ, TS, SQ, SQ
    if kind in ("relu_inplace", "relu_inplace_tile", "bf16_relu_inplace"):
        return footprint_out(v)
    if kind == "identity_window":
        return a, 0, FM, WIN, FN
    if kind == "bf16_identity_window":
        return a, 0, SQ, HWIN, SQ
    if kind == "add_bcast_col_tile":
        return VB, tj * TS, 1, TS, TS
    return None


class CoherenceProgram:
    def __init__(self, seed, device, hooks):
        """device: the backend under test; hooks: the object with the synchronisation / mode calls (the runtime)"""
        self.seed, self.dev, self.rt = seed, device, hooks
        self.model = OracleBackend()
        self.rng = np.random.default_rng(seed)
        self.buf = [CohBuf(*b) for b in BUFS]
        for b in self.buf:
            b.write(0, self.small(b.n))
        self.acc = [0] * len(BUFS)
        self.step, self.log, self.other_stream, self.stream = 0, [], False, None

    def small(self, n=None):
        return self.rng.integers(-3, 4, n)

    def below(self, n):
        return int(self.rng.integers(0, n))

    def note(self, text):
        self.log.append("  step %d: %s" % (self.step, text))
        self.step += 1
        COH["steps"] += 1

    def where(self):
        return "coherence program seed %d, step %d; the last steps:\n%s" % (self.seed, self.step - 1, "\n".join(self.log[-14:]))

    def check(self):
        COH["checks"] += 1
        for b in self.buf:
            if not np.array_equal(b.raw, b.sraw):
                i = int(np.flatnonzero(b.raw != b.sraw)[0])
                e = (i - b.OFF) // b.a.itemsize
                inside = 0 <= e < b.n
                raise AssertionError("buffer %s differs from the oracle's shadow at mapping byte %d (element %d of %d: host %r, oracle %r) in %s" % (
                    b.name, i, e, b.n, float(ed.as_f32(b.a[e:e + 1])[0]) if inside else None, float(ed.as_f32(b.s[e:e + 1])[0]) if inside else None, self.where()))

    # ---- what an invoke needs to stay exact
    def eligible(self, v):
        kind, a, b, c, ti, tj, beta1 = v
        B = self.buf
        if kind in ("brgemm", "fused_brgemm"):
            if c in (a, b):
                return False
            if np.abs(B[a].model(0, SQ, SQ, SQ)).max() > IN_MAX or np.abs(B[b].model(0, SQ, SQ, SQ)).max() > IN_MAX:
                return False
            return not beta1 or self.acc[c] < MAX_ACCUMULATIONS
        if kind == "bf16_brgemm":
            return not beta1 or self.acc[c] < MAX_ACCUMULATIONS
        if kind == "brgemm_tile":
            return np.abs(B[a].model(ti * TS * SQ, TS, SQ, SQ)).max() <= IN_MAX and (not beta1 or self.acc[FL] < MAX_ACCUMULATIONS)
        if kind == "add_bcast_col":
            return self.acc[c] < MAX_ACCUMULATIONS
        if kind == "add_bcast_col_tile":
            return self.acc[FL] < MAX_ACCUMULATIONS
        return True

    def assert_exact(self, v, operands):
        """the precondition of the bit-exact comparison, on the MODEL's values: integers, and every sum below 2^24"""
        kind, a, b, c, ti, tj, beta1 = v
        if kind not in ("brgemm", "fused_brgemm", "brgemm_tile", "bf16_brgemm", "add_bcast_col", "add_bcast_col_tile"):
            return
        B = self.buf
        vals = []
        if kind in ("add_bcast_col", "add_bcast_col_tile"):
            o = footprint_out(v)
            vals = [B[a].model(o[1] if kind.endswith("tile") else 0, o[2], o[3], o[4]), B[VB].model(tj * TS if kind.endswith("tile") else 0, 1, o[3], o[3])]
            bound = np.abs(vals[0]).max() + np.abs(vals[1]).max()
        else:
            m = TS if kind == "brgemm_tile" else SQ
            A = B[a].model(operands[0][1], m, SQ, SQ)  # both batch elements: columns 0 .. 63 of the rows
            ldb = FN if kind == "brgemm_tile" else SQ
            Bm = B[b].model(operands[1][1], SQ, m, ldb)
            o = footprint_out(v)
            Cm = B[c].model(o[1], o[2], o[3], o[4]) if beta1 else np.zeros(1)
            Vm = B[VB].model(0, 1, SQ, SQ) if kind == "fused_brgemm" else np.zeros(1)
            vals = [A, Bm, Cm, Vm]
            bound = KB * BR * np.abs(A).max() * np.abs(Bm).max() + np.abs(Cm).max() + np.abs(Vm).max()
            if kind == "bf16_brgemm":
                assert np.abs(A).max() < 2 ** 8 and np.abs(Bm).max() < 2 ** 8, self.where()
        for x in vals:
            assert np.array_equal(x, np.floor(x)), "a model value is not an integer in " + self.where()
        assert bound < 2 ** 24, "exactness precondition broken (bound %g) in %s" % (bound, self.where())

    def issue(self, v):
        kind, a, b, c, ti, tj, beta1 = v
        o = footprint_out(v)
        if kind == "brgemm":
            op, operands = "whole%d" % beta1, [(a, 0), (b, 0), (c, 0)]
        elif kind == "fused_brgemm":
            op, operands = "fused%d" % beta1, [(a, 0), (b, 0), (c, 0), (VB, 0)]
        elif kind == "bf16_brgemm":
            op, operands = "hgemm%d" % beta1, [(a, 0), (b, 0), (c, 0)]
        elif kind == "brgemm_tile":
            op, operands = "tile%d" % beta1, [(a, ti * TS * SQ), (WI, tj * TS), (c, o[1])]
        elif kind in ("relu_inplace", "relu_inplace_tile", "bf16_relu_inplace"):
            op, operands = {"relu_inplace": "relu_sq", "relu_inplace_tile": "relu_tile", "bf16_relu_inplace": "hrelu"}[kind], [(c, o[1]), (c, o[1])]
        elif kind in ("zero", "zero_tile", "bf16_zero_tile"):
            op, operands = {"zero": "zero_sq", "zero_tile": "zero_tile", "bf16_zero_tile": "hzero_tile"}[kind], [(c, o[1]), (c, o[1])]
        elif kind in ("identity_window", "bf16_identity_window"):
            op, operands = ("ident_win" if kind == "identity_window" else "hident_win"), [(a, 0), (c, o[1])]
        elif kind == "add_bcast_col":
            op, operands = "add_sq", [(a, 0), (VB, 0), (c, 0)]
        else:
            op, operands = "add_tile", [(FL, o[1]), (VB, tj * TS), (c, o[1])]
        self.note("invoke %s (%s) a=%s b=%s out=%s tile (%d,%d) beta %d" % (kind, op, BUFS[a][0] if a >= 0 else "-", BUFS[b][0] if b >= 0 else "-", BUFS[c][0], ti, tj, beta1))
        self.assert_exact(v, operands)
        COH["invokes"] += 1
        COH["kinds"][kind] = COH["kinds"].get(kind, 0) + 1
        br = BR
        self.dev.run(op, [(self.buf[i].a, off) for i, off in operands], br)
        self.model.run(op, [(self.buf[i].s, off) for i, off in operands], br)
        if beta1 and kind in ("brgemm", "fused_brgemm", "brgemm_tile", "bf16_brgemm") or kind.startswith("add_"):
            self.acc[c] += 1
        elif kind in ("brgemm", "fused_brgemm", "bf16_brgemm", "zero"):
            self.acc[c] = 0

    def random_inv(self):
        while True:
            kind = INVOKE_KINDS[self.below(len(INVOKE_KINDS))]
            a = b = -1
            ti, tj, beta1 = self.below(2), self.below(FN // TS), self.below(2)
            sq = lambda: S0 + self.below(4)  # noqa: E731
            if kind in ("brgemm", "fused_brgemm"):
                a, b, c = sq(), sq(), sq()
            elif kind == "bf16_brgemm":
                a, b, c = HA, HB, HC
            elif kind == "brgemm_tile":
                a, b, c = sq(), WI, FL
            elif kind in ("relu_inplace", "zero"):
                c = sq()
            elif kind in ("relu_inplace_tile", "zero_tile"):
                c = FL
            elif kind == "identity_window":
                a, c = WI, FL
            elif kind == "add_bcast_col":
                a, b, c = sq(), VB, sq()
            elif kind == "add_bcast_col_tile":
                a, b, c = FL, VB, FL
            elif kind == "bf16_relu_inplace":
                c = H0 + self.below(2)
            elif kind == "bf16_identity_window":
                a, c = H0, H1
            else:
                c, tj = H0 + self.below(2), self.below(2)
            if kind == "zero" and self.below(3):
                continue  # (rarely: it wipes a whole buffer)
            v = (kind, a, b, c, ti, tj, beta1)
            if self.eligible(v):
                return v

    # ---- host edits (the model follows): one element, a run of a few pages, a range written by a system call
    def edit_element(self, b, i):
        x = self.buf[b]
        nv = int(self.small())
        if nv == float(ed.as_f32(x.s[i:i + 1])[0]):
            nv = -3 if nv == 3 else nv + 1
        self.note("host edit: %s[%d] = %d" % (x.name, i, nv))
        x.write(i, [nv])
        COH["edits"] += 1

    def edit_run(self, b, lo, cnt):
        x = self.buf[b]
        cnt = min(cnt, x.n - lo)
        self.note("host edit: %s[%d .. %d) refilled" % (x.name, lo, lo + cnt))
        x.write(lo, self.small(cnt))
        COH["edits"] += 1

    def edit_syscall(self, b, lo, cnt):
        x = self.buf[b]
        cnt = min(cnt, x.n - lo)
        self.note("host edit: read(2) of %d bytes into %s[%d ..)" % (cnt * x.a.itemsize, x.name, lo))
        with open("/dev/zero", "rb", buffering=0) as z:
            got = z.readinto(memoryview(x.a[lo:lo + cnt]).cast("B"))  # the kernel writes the operand's pages
        assert got == cnt * x.a.itemsize
        x.s[lo:lo + cnt] = 0
        COH["edits"] += 1

    def random_edit(self):
        b = self.below(len(BUFS))
        x = self.buf[b]
        how, lo = self.below(3), self.below(x.n)
        if how == 0:
            self.edit_element(b, lo)
        elif how == 1:
            self.edit_run(b, lo, 1024 + self.below(2048))  # (f32: one to three pages)
        else:
            self.edit_syscall(b, lo, 512 + self.below(2048))

    def reinit_large(self):
        """GEMM inputs that outgrew IN_MAX (they were outputs) and outputs that accumulated often are written afresh by the host"""
        for b in (S0, S1, S2, S3):
            if (np.abs(self.buf[b].model(0, SQ, SQ, SQ)).max() > IN_MAX or self.acc[b] >= MAX_ACCUMULATIONS) and self.below(3):
                self.edit_run(b, 0, self.buf[b].n)
                self.acc[b] = 0
        for b in (FL, HC):
            if self.acc[b] >= MAX_ACCUMULATIONS:
                self.edit_run(b, 0, self.buf[b].n)
                self.acc[b] = 0

    def sync_point(self, kind, t0):
        self.note("synchronisation point: " + SYNC_KINDS[kind])
        COH["syncs"] += 1
        rt = self.rt
        if kind == 0:
            rt.synchronize()
        elif kind == 1:
            rt.perf_stop_timer(t0)
        elif kind == 2:
            rt.set_async(False)
            rt.set_async(True)
        elif kind == 3:
            self.other_stream = not self.other_stream
            rt.set_stream(self.stream if self.other_stream else None)
        else:
            rt.set_host_cache(False)
            assert rt.set_host_cache(True) == 0

    def run(self, other_stream):
        rt, self.stream = self.rt, other_stream
        COH["programs"] += 1
        rt.set_async(False)
        rt.set_tile_queue(0)
        prev, prev_kind, prev_async, is_async = [], -1, False, False
        try:
            for seg in range(7 + self.below(4)):
                mode = self.below(5)  # 0: synchronous, 1-2: asynchronous, 3-4: asynchronous + tile queue
                endkind = (self.seed + seg) % len(SYNC_KINDS)
                mine = []
                if mode == 0:
                    if is_async:
                        rt.set_async(False)
                    is_async = False
                    self.note("segment %d: synchronous" % seg)
                    t0 = rt.perf_start_timer()
                    for _ in range(4 + self.below(5)):
                        if self.below(3) == 0:
                            self.reinit_large()
                            self.random_edit()
                            continue
                        v = prev[self.below(len(prev))] if prev and self.below(2) else self.random_inv()
                        if not self.eligible(v):
                            v = self.random_inv()
                        self.issue(v)
                        mine.append(v)
                        self.check()  # results visible on return
                    if endkind != 2 and self.below(2):
                        self.sync_point(endkind, t0)
                        self.check()
                    prev_async = False
                else:
                    queue = int(mode >= 3)
                    rt.set_async(True)
                    rt.set_tile_queue(queue)
                    is_async = True
                    self.note("segment %d: asynchronous, tile queue %d, behind %s" % (seg, queue, SYNC_KINDS[prev_kind] if prev_kind >= 0 else "the start"))
                    t0 = rt.perf_start_timer()
                    # host phase: directly behind the synchronisation point, before the segment's first invoke
                    self.reinit_large()
                    for _ in range(self.below(3)):
                        self.random_edit()
                    plan, half = [], [False, False, False]
                    if prev_async and prev:
                        want = 1 + self.below(3)  # bit 0: edit-then-invoke, bit 1: rewrite-an-output
                        if want & 1:  # the host edits an element that an invoke of the last segment read (its mirror exists); it runs again
                            v = prev[self.below(len(prev))]
                            f = footprint_in(v)
                            if f is not None and self.eligible(v):
                                self.edit_element(f[0], f[1] + self.below(f[2]) * f[4] + self.below(f[3]))
                                if self.eligible(v):
                                    plan.append(v)
                                    half[0] = True
                        if want & 2:  # an invoke of the last segment writes its output again; the host scribbles on it first, so that
                            #           a write-back that does not happen shows
                            v = prev[self.below(len(prev))]
                            if v[0] in GEMM_KINDS and self.below(3):  # ... as the C of a beta-1 invoke, which READS the host's edit
                                v1 = v[:6] + (1,)
                                if self.eligible(v1):
                                    v = v1
                            f = footprint_out(v)
                            if self.eligible(v):
                                self.edit_element(f[0], f[1] + self.below(f[2]) * f[4] + self.below(f[3]))
                                if self.eligible(v):
                                    plan.append(v)
                                    half[1] = True
                                    half[2] = v[0] in GEMM_KINDS and v[6] == 1
                    for v in plan:
                        if self.eligible(v):
                            self.issue(v)
                            mine.append(v)
                        else:
                            half = [False, False, False]  # (an earlier invoke of the plan changed what this one needs: not counted)
                    for _ in range(2 + self.below(5)):
                        v = mine[self.below(len(mine))] if mine and self.below(3) == 0 else self.random_inv()
                        if not self.eligible(v):
                            v = self.random_inv()
                        self.issue(v)
                        mine.append(v)
                    self.sync_point(endkind, t0)
                    self.check()
                    if prev_kind >= 0:
                        for hf in (0, 1, 2):
                            if half[hf]:
                                key = (SYNC_KINDS[prev_kind], HALVES[hf], queue)
                                COH["pair"][key] = COH["pair"].get(key, 0) + 1
                    prev_async, prev_kind = True, endkind
                prev = mine
        finally:
            rt.set_stream(None)
            rt.set_tile_queue(0)
            rt.set_async(False)
        self.check()


_other_stream = []


@pytest.mark.parametrize("seed", COH_SEEDS)
def test_coherence_program_matches_the_oracle_shadow(rt_cache, seed):
    """one seeded program (see above); a failure names the seed, the step and the last steps, so it replays"""
    import torch
    if not _other_stream:
        _other_stream.append(torch.cuda.Stream())
    if COH["stats0"] is None:
        COH["stats0"] = rt_cache.host_cache_stats()
    p = CoherenceProgram(seed, RuntimeBackend(rt_cache), rt_cache)
    p.run(_other_stream[0])
    rt_cache.set_host_cache(False)  # "switching it off writes everything back"
    p.check()
    rt_cache.set_host_cache(True)
    COH["stats1"] = rt_cache.host_cache_stats()


def test_zz_coherence_coverage(rt_cache):
    """runs behind the programs: every (synchronisation kind) x (edit-then-invoke, rewrite-an-output, a host edit of an output that a
    beta-1 invoke then reads) occurred in asynchronous mode
    with the tile queue off and on, every invoke kind ran on host pointers with the cache on, the cache translated invokes on its
    lock-free path and skipped no write-back - a run in which it had quietly given every extent up would pass the byte checks"""
    print("[coherence] %(programs)d programs, %(steps)d steps (%(invokes)d invokes, %(edits)d host edits, %(syncs)d synchronisation points, "
          "%(checks)d whole-memory checks)" % COH)
    missing = []
    for k in SYNC_KINDS:
        row = []
        for hf in HALVES:
            for q in (0, 1):
                n = COH["pair"].get((k, hf, q), 0)
                row.append("%s queue %d: %d" % (hf, q, n))
                if not n:
                    missing.append((k, hf, q))
        print("[coherence] behind %-24s %s" % (k, "; ".join(row)))
    print("[coherence] invoke kinds: %s" % ", ".join("%s %d" % (k, COH["kinds"].get(k, 0)) for k in INVOKE_KINDS))
    missing += [k for k in INVOKE_KINDS if not COH["kinds"].get(k)]
    assert COH["programs"] == len(COH_SEEDS), "the programs did not all run: %d of %d" % (COH["programs"], len(COH_SEEDS))
    assert not missing, "not reached: %s" % missing
    s0, s1 = COH["stats0"], COH["stats1"]
    print("[coherence] lock-free translations %d, uploaded %d B, written back %d B, pages not written back %d" % (
        s1["fast_invokes"] - s0["fast_invokes"], s1["uploaded_bytes"] - s0["uploaded_bytes"], s1["written_back_bytes"] - s0["written_back_bytes"],
        s1["pages_not_written_back"] - s0["pages_not_written_back"]))
    assert s1["fast_invokes"] - s0["fast_invokes"] > 0, (s0, s1)
    assert s1["pages_not_written_back"] - s0["pages_not_written_back"] == 0, (s0, s1)
    assert s1["written_back_bytes"] > s0["written_back_bytes"] and s1["uploaded_bytes"] > s0["uploaded_bytes"], (s0, s1)


# ---------------------------------------------------------------- the size edges of the copy paths
# copy_back / upload / the scratch output of complete() around Staging::SLOT (4 MiB): one unary identity (or an in-place relu) per case,
# so the expected bytes need no arithmetic. The output's mapping holds a sentinel the host wrote: the gaps between rows and the guard
# bytes behind the last row must keep it. (rows, row_bytes, pitch) of the OUTPUT in bytes; the same list as tests/hostcache/driver.cpp.
SLOT = 4 << 20
EDGE_CASES = (
    ("wide rows, pitch just below a slot", 3, SLOT - 256, SLOT - 64, 1, False),
    ("wide rows, pitch == slot", 3, SLOT - 128, SLOT, 1, False),
    ("wide rows, pitch just above a slot", 3, SLOT - 64, SLOT + 64, 1, False),
    ("wide rows, row and pitch above a slot", 3, SLOT + 64, SLOT + 256, 1, False),
    ("wide rows, pitch 5.2 MB", 4, 4800000, 5200000, 1, False),
    ("one wide row behind a pitch above a slot", 1, 4800000, 5200000, 1, False),
    ("wide rows, one slot and a remainder in all", 17, 262144, 262208, 1, False),
    ("wide rows, two slots and a remainder in all", 33, 262144, 262208, 1, False),
    ("wide rows, three slots and a remainder in all", 49, 262144, 262208, 1, False),
    ("narrow rows, row just below a slot", 2, SLOT - 64, 4 * SLOT + 64, 1, False),
    ("narrow rows, row == slot", 2, SLOT, 4 * SLOT + 64, 1, False),
    ("narrow rows, row just above a slot", 2, SLOT + 64, 4 * SLOT + 512, 1, False),
    ("narrow rows, row 4.4 MB", 3, 4400000, 18400000, 1, False),
    ("narrow rows, rows x row_bytes cross a slot", 17, 262144, 4 * 262144 + 64, 1, False),
    ("branch boundary, row_bytes x 4 == pitch (not narrow)", 1100, 4000, 16000, 1, False),
    ("branch boundary, row_bytes x 4 + 4 == pitch (narrow)", 1100, 4000, 16004, 1, False),
    ("dense output of two slots and a half, unaligned ends", 1, 10 * 1048576 + 1000, 10 * 1048576 + 1000, 1, False),
    ("dense in-place relu of two slots and a half", 1, 10 * 1048576 + 1000, 10 * 1048576 + 1000, 5, False),
    ("input of two slots and a half, first - middle - last page edited", 1, 10 * 1048576 + 1000, 10 * 1048576 + 1000, 1, True),
)


def edge_values(n, dtype):
    i = np.arange(n, dtype=np.int64)
    if dtype == np.float32:
        return ((i % 1021) - 400).astype(np.float32)
    return orc.f32_to_bf16(((i % 251) - 100).astype(np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=["f32", "bf16"])
@pytest.mark.parametrize("is_async", [False, True], ids=["sync", "async"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0].replace(" ", "_") for c in EDGE_CASES])
def test_copy_path_size_edges(rt_cache, case, is_async, dtype):
    import mmap
    rt = rt_cache
    what, m, row_bytes, pitch, op, edit_input = case
    es = np.dtype(dtype).itemsize
    n, ld = row_bytes // es, pitch // es
    dt = F32 if dtype == np.float32 else BF16
    OFF, GUARD = 256, 8192
    inplace = op == 5
    in_bytes, out_bytes = m * n * es, ((m - 1) * ld + n) * es
    xm = mmap.mmap(-1, (OFF + in_bytes + GUARD + 4095) // 4096 * 4096)
    xraw = np.frombuffer(xm, dtype=np.uint8)
    xraw[:] = 0x5A
    X = xraw[OFF:OFF + in_bytes].view(dtype)
    X[:] = edge_values(m * n, dtype)
    if inplace:
        oraw = xraw
    else:
        om = mmap.mmap(-1, (OFF + out_bytes + GUARD + 4095) // 4096 * 4096)
        oraw = np.frombuffer(om, dtype=np.uint8)
        oraw[:] = 0x5A
    O = oraw[OFF:OFF + out_bytes].view(dtype)
    h = rt.unary_dispatch(op, dt, m, n, n, ld, 0)
    try:
        rt.set_async(is_async)
        for pass_ in range(2 if edit_input else 1):
            if pass_ == 1:  # the host edits the first, one middle and the last page of the input, directly behind the synchronisation point
                X[1], X[m * n // 2], X[m * n - 2] = edge_values(10000, dtype)[[7777, 8888, 9999]]
                oraw[:] = 0x5A
            want = np.full(oraw.size, 0x5A, np.uint8)
            src = X.copy()
            if inplace:
                f = ed.as_f32(src)
                src[~(f > 0)] = 0
                want[OFF:OFF + in_bytes] = src.view(np.uint8)
            else:
                for r in range(m):
                    want[OFF + r * pitch:OFF + r * pitch + row_bytes] = src[r * n:(r + 1) * n].view(np.uint8)
            rt.unary(dt, h, X, 0, O, 0)
            if is_async:
                rt.synchronize()
            bad = np.flatnonzero(oraw != want)
            assert bad.size == 0, "%s (pass %d): %d wrong bytes of the output's mapping, the first at byte %d (row pitch %d, data from byte %d)" % (
                what, pass_, bad.size, int(bad[0]), pitch, OFF)
    finally:  # (also behind a failed assertion: the next case must not inherit asynchronous mode or mirrors of mappings that are gone)
        rt.set_async(False)
        rt.set_host_cache(False)
        rt.set_host_cache(True)
