"""Worker of tests/test_graph_capture_gpu.py, and the helpers the test shares with it. As a program (its own process: the tile queue's slot
ring, its trace cache and the scratch blocks of the split kernels are per process and never freed - a test in the main process that used
them up would change what later tests run on):
  graph_capture_worker.py queue cold     a group of 16 tile invokes of one 32x32x32 descriptor, ended by a flush, captured into a graph
                                         with no warm-up: the flush gathers the members into a pinned slot of the ring
  graph_capture_worker.py queue warm     the same after three warm-up iterations: the whole group replays from its segment's device list;
                                         a second, never-seen group of 6 in the same capture takes the pinned slot
  graph_capture_worker.py small          a group of 6 bf16 tile invokes under a forced split count (the split of brgemm_bf16_small.hip lives in
                                         grouped launches): captured it runs and reports the unsplit kernel, un-captured the split one
  graph_capture_worker.py growth         three skinny split calls back to back on one stream: the second outgrows the stream's first
                                         scratch block (tpp-mlir_amd/csrc/split_scratch.h)
  graph_capture_worker.py streams        a forced-split skinny call on the default stream and on seventeen more: the 17th (device, stream)
                                         pair gets no block and runs unsplit
Each prints one JSON line and exits 0; "errors" lists what did not hold (the test asserts it is empty).

queue: the captured flush is the eighth of its slot group (seven flushes of smaller groups come first), so TileQueue::launched would record
the group's completion event inside the capture. Before each of the three replays at least 40 un-captured flushes of OTHER groups of the same
descriptor - groups below MIN_SEG = 16 invokes, which always gather into a pinned slot: every ring slot is rewritten and every event group
is entered again - interleaved with groups of 16 that are recorded and replayed whole (more than NSEG = 64 of them before the first
replay: the captured group's segment is evicted and its work-list buffers travel to another group). Every buffer a work list ever named
stays allocated until the process ends: a stale list can only give wrong bits in live memory. Each replay runs on fresh exact inputs and
NaN-filled outputs and must give the oracle's bits; the other groups' inputs are overwritten before the replay, so a replay that ran
one of THEIR work lists would change their outputs - which must still hold what their own runs wrote."""
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
from oracle import pyoracle as orc  # noqa: E402
from skinny_bf16_worker import Case  # noqa: E402
from skinny_bf16_worker import text as skinny_text  # noqa: E402
from skinny_split_worker import expected_split_stats  # noqa: E402
from skinny_split_worker import text as split_text  # noqa: E402

F32, BF16 = 1, 2
NSEG, MIN_SEG, SLOTS, GROUP, SPLIT_MAX_BLOCKS = 64, 16, 32, 8, 16  # rt_tile_queue.h TileQueue, split_scratch.h


def captured(rt, fn, warm=1):
    """fn() on a side stream the way tests/test_chain_gpu.py captures: `warm` times un-captured, then once inside a capture (one stream,
    a linear graph). Returns the graph, what fn returned inside the capture, and the stream; the runtime is back on the default stream"""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.stream(s):
            rt.set_stream(s)
            for _ in range(warm):
                fn()
            rt.synchronize()
            s.synchronize()
            with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
                inside = fn()
    finally:
        rt.set_stream(None)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    return g, inside, s


class F32Case:
    """One whole-layer f32 call on exact inputs, with the interface of dma256_images_worker.Case: br batch elements, each k wide, of a
    row-major A and B. Strided like that class: a gap of 8 columns behind every batch element of an A row and 4 more behind the row, two
    k-rows between the batch elements of B and 4 columns behind its rows, 12 behind the rows of C, every base pointer moved by 16 bytes.
    NaN / +inf / -inf in everything the descriptor does not name, a bit pattern around the C window."""

    def __init__(self, m, n, k, br, seed, beta0=False, bias=True, relu=True):
        self.image, self.m, self.n, self.k, self.br = None, m, n, k, br
        self.beta0, self.bias, self.relu = beta0, bias, relu
        self.lda, self.sa, self.ldb, self.ldc, self.offs = br * (k + 8) + 4, k + 8, n + 4, n + 12, (4, 8, 4, 4)
        self.sb = (k + 2) * self.ldb
        o = self.offs
        sizes = (o[0] + (br - 1) * self.sa + m * self.lda + 8, o[1] + (br - 1) * self.sb + k * self.ldb + 2 * self.ldb + 8, o[2] + m * self.ldc + 8, o[3] + n + 8)
        rng = np.random.default_rng(seed)
        ra, rb, rc = ed.exact_ranges(F32, k * br)
        assert k * br * ra * rb + 2 * rc * (1 + 2.0 ** -8) < 2 ** 24
        self.A, self.B, self.C, self.D = (ed.exact_fill(rng, s, F32, r) for s, r in zip(sizes, (ra, rb, rc, rc)))
        ii, jj = np.arange(m)[:, None], np.arange(n)[None, :]
        self.win = (o[2] + ii * self.ldc + jj).reshape(-1)
        la, lb, _, ld_ = ed.live_masks(sizes, m, n, k, br, self.lda, self.ldb, self.ldc, self.sa, self.sb, o, beta0=beta0, bias=bias)
        for arr, lv in zip((self.A, self.B, self.D), (la, lb, ld_)):
            arr[~lv] = ed.poison_fill(arr.size, F32)[~lv]
        keep = self.C[self.win].copy()
        self.C[:] = (((np.arange(sizes[2], dtype=np.uint64) * 2654435761 + 12345) & 0x00FFFFFF) | 0x3F000000).astype(np.uint32).view(np.float32)  # a (finite) bit pattern around C
        self.C[self.win] = np.nan if beta0 else keep

    def fused(self):
        return self.bias or self.relu

    def args(self):
        return (F32, self.m, self.n, self.k, self.lda, self.ldb, self.ldc, self.sa, self.sb, 4 if self.beta0 else 0)

    def fp64(self):
        """the result in fp64 (exact inputs: every intermediate is an integer below 2^24, so f32 arithmetic in any order rounds nothing)"""
        m, n, k, o = self.m, self.n, self.k, self.offs
        ii, kk, jj = np.arange(m)[:, None], np.arange(k)[None, :], np.arange(n)[None, :]
        acc = np.zeros((m, n)) if self.beta0 else self.C[self.win].astype(np.float64).reshape(m, n)
        for b in range(self.br):
            a = self.A[(o[0] + b * self.sa + ii * self.lda + kk).reshape(-1)].astype(np.float64).reshape(m, k)
            w = self.B[(o[1] + b * self.sb + np.arange(k)[:, None] * self.ldb + jj).reshape(-1)].astype(np.float64).reshape(k, n)
            acc = acc + a @ w
        if self.bias:
            acc = acc + self.D[o[3]:o[3] + n].astype(np.float64)[None, :]
        if self.relu:
            acc = np.maximum(acc, 0)
        return acc.astype(np.float32).reshape(-1)

    def oracle(self):
        ref, o = self.C.copy(), self.offs
        if self.fused():
            orc.fused_brgemm(*self.args(), 0, 5 if self.relu else 0, 4 if self.bias else 0, 1 if self.bias else 0, self.A, o[0], self.B, o[1], ref, o[2],
                             self.D, o[3], self.br)
        else:
            orc.brgemm(*self.args(), self.A, o[0], self.B, o[1], ref, o[2], self.br)
        return ref

    def dispatch(self, rt, force=None):
        if force is not None:
            rt.force_variant(force)
        try:
            if self.fused():
                return rt.fused_brgemm_dispatch(*self.args(), 0, 5 if self.relu else 0, 4 if self.bias else 0, 1 if self.bias else 0)
            return rt.brgemm_dispatch(*self.args())
        finally:
            if force is not None:
                rt.force_variant(-1)

    def device(self):
        import torch
        return [torch.from_numpy(x.copy()).cuda() for x in (self.A, self.B, self.C, self.D)]

    def outside_untouched(self, got):
        mask = np.ones(self.C.size, bool)
        mask[self.win] = False
        return np.array_equal(ed.bits(got)[mask], ed.bits(self.C)[mask])


def dtype_of(case):
    return F32 if case.image is None else BF16


def upload(bufs, case):
    """the case's host operands into the device buffers of another case of the same shape, in place (C: its poison and bit pattern)"""
    import torch
    for d, h in zip(bufs, (case.A, case.B, case.C, case.D)):
        d.copy_(torch.from_numpy(h.view(np.int16) if h.dtype == np.uint16 else h))


def download(buf, case):
    a = buf.cpu().numpy()
    return a.view(np.uint16) if case.C.dtype == np.uint16 else a


def invoke(rt, case, h, bufs):
    dA, dB, dC, dD = bufs
    o = case.offs
    if case.bias or case.relu:
        rt.fused_brgemm(dtype_of(case), h, dA, o[0], dB, o[1], dC, o[2], dD, o[3], case.br)
    else:
        rt.brgemm(dtype_of(case), h, dA, o[0], dB, o[1], dC, o[2], case.br)
    return rt.last_refined_kernel()


def same_bits(a, b):
    return np.array_equal(ed.bits(a), ed.bits(b))


# ------------------------------------------------------------------------------------------------ the tile queue in a capture
KB = 2  # batch elements of a tile invoke: k = 64 per output, A and B integers up to 255 - every sum an integer below 2^24


class TileGroup:
    """mb x nb invokes of the 32x32x32 descriptor (beta 0; f32, or bf16 with a VNNI-2 B) over packed blocks, mlir-gen's layout and the
    pattern of tests/test_tile_queue_gpu.py test_packed_mlp_layers_tile_invokes: A [mb][kb][32][32], B [nb][kb][32][32], C [mb][nb][32][32] -
    never a tile grid over flat operands, so a whole replay launches from the work list. Behind C a guard tile with a bit pattern."""

    def __init__(self, mb, nb, seed, dt=F32, kb=KB):
        self.mb, self.nb, self.seed, self.dt, self.kb = mb, nb, seed, dt, kb
        self.flags = 4 | (2048 if dt == BF16 else 0)
        if dt == F32:
            self.C0 = np.full((mb * nb + 1) * 1024, np.nan, np.float32)
            self.C0[mb * nb * 1024:] = (((np.arange(1024, dtype=np.uint64) * 40503 + seed) & 0x007FFFFF) | 0x3F800000).astype(np.uint32).view(np.float32)
        else:
            self.C0 = np.full((mb * nb + 1) * 1024, ed.BF16_NAN, np.uint16)
            self.C0[mb * nb * 1024:] = (((np.arange(1024, dtype=np.uint64) * 40503 + seed) & 0x007F) | 0x3F80).astype(np.uint16)
        self.fresh(seed)
        self.dA, self.dB, self.dC = dev(self.A), dev(self.B), dev(self.C0)

    def fresh(self, seed):
        rng = np.random.default_rng(seed)
        ra, rb, _ = ed.exact_ranges(self.dt, 32 * self.kb)
        assert 32 * self.kb * ra * rb < 2 ** 24
        self.A, self.B = ed.exact_fill(rng, self.mb * self.kb * 1024, self.dt, ra), ed.exact_fill(rng, self.nb * self.kb * 1024, self.dt, rb)

    def upload(self, outputs=True):
        self.dA.copy_(dev(self.A))
        self.dB.copy_(dev(self.B))
        if outputs:
            self.dC.copy_(dev(self.C0))

    def invoke(self, rt, h):
        kb = self.kb
        for i in range(self.mb):
            for j in range(self.nb):
                rt.brgemm(self.dt, h, self.dA, i * kb * 1024, self.dB, j * kb * 1024, self.dC, (i * self.nb + j) * 1024, kb)

    def oracle(self):
        ref, kb = self.C0.copy(), self.kb
        for i in range(self.mb):
            for j in range(self.nb):
                orc.brgemm(self.dt, 32, 32, 32, 32, 32, 32, 1024, 1024, self.flags, self.A, i * kb * 1024, self.B, j * kb * 1024, ref, (i * self.nb + j) * 1024, kb)
        assert np.isfinite(ed.as_f32(ref)).all()
        return ref

    def got(self):
        a = self.dC.cpu().numpy()
        return a.view(np.uint16) if self.dt == BF16 else a


def dev(a):
    import torch
    return torch.from_numpy((a.view(np.int16) if a.dtype == np.uint16 else a).copy()).cuda()


SMALL = [(1, 3), (2, 2), (3, 3), (2, 5), (3, 4), (1, 7), (3, 5), (2, 7)]  # groups below MIN_SEG invokes: never recorded, always a pinned slot
BIG = [(4, 4), (4, 5), (5, 4), (3, 6)]                                   # MIN_SEG invokes and more: recorded, the second run replays whole


def queue_scenario(rt, warm):
    import torch
    errors = []
    rt.set_async(True)
    rt.set_tile_queue(1)
    h = rt.brgemm_dispatch(F32, 32, 32, 32, 32, 32, 32, 1024, 1024, 4)
    keep = []       # every group ever queued: its buffers stay allocated until the process ends
    seeds = iter(range(1000, 100000))
    stats0 = rt.tile_queue_stats()

    def other(shape):
        g = TileGroup(shape[0], shape[1], next(seeds))
        keep.append(g)
        return g

    def run(g):
        g.invoke(rt, h)
        rt.flush()

    cap = TileGroup(4, 4, 7)  # MIN_SEG invokes: the capture's cold pass records it as a segment, the warm one replays it whole
    assert cap.mb * cap.nb >= MIN_SEG
    extra = TileGroup(2, 3, 8) if warm else None  # warm: a group the queue has never seen, in the same capture - it takes the pinned slot

    def step():
        cap.invoke(rt, h)
        rt.flush()
        if extra is not None:
            extra.invoke(rt, h)
            rt.flush()

    # Everything up to the end of the capture on ONE side stream. The ring position: the captured slot-taking flush must be the eighth of
    # its slot group. Cold: seven flushes of small groups first. Warm: six, and the first of the three warm-up iterations of the captured
    # group ALONE takes the seventh slot (it records the group; the next two replay whole and take none; the extra group stays unseen).
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.stream(s):
            rt.set_stream(s)
            for i in range(GROUP - 1 - (1 if warm else 0)):
                run(other(SMALL[i % len(SMALL)]))
            before = rt.tile_queue_stats()
            for _ in range(3 if warm else 0):
                cap.invoke(rt, h)
                rt.flush()
            rt.synchronize()
            s.synchronize()
            mid = rt.tile_queue_stats()
            with torch.cuda.graph(graph, stream=s, capture_error_mode="relaxed"):
                step()
    finally:
        rt.set_stream(None)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    # launches, invokes with full bookkeeping, invokes replayed of the warm-up: the group recorded once and replayed whole twice
    if warm and [x - y for x, y in zip(mid[:3], before[:3])] != [3, 16, 32]:
        errors.append("warm-up: the group was not recorded once and replayed twice: %r -> %r" % (before, mid))
    before = mid
    after = rt.tile_queue_stats()
    in_capture = [a - b for a, b in zip(after, before)]
    cap_groups = [cap] + ([extra] if extra is not None else [])

    flushes = slot_flushes = big_seen = 0
    replays = []
    for rep in range(3):
        phase = []
        n_big = NSEG + 6 if rep == 0 else 10
        n_small = 40 + 3 * rep  # (the count varies: the ring position of the captured slot's next use differs from phase to phase)
        bi = si = 0
        while bi < n_big or si < n_small:
            if si < n_small:
                g = other(SMALL[(si + rep) % len(SMALL)])
                run(g)
                phase.append(g)
                si += 1
                flushes += 1
                slot_flushes += 1
            if bi < n_big:
                g = other(BIG[(bi + rep) % len(BIG)])
                run(g)  # recorded (a pinned slot)
                run(g)  # replayed whole from the segment's device list: the list is built now, in buffers that may have been another segment's
                phase.append(g)
                bi += 1
                big_seen += 1
                flushes += 2
                slot_flushes += 1
        rt.synchronize()
        torch.cuda.synchronize()
        want = [g.oracle() for g in phase]
        for g, w in zip(phase, want):
            if not same_bits(g.got(), w):
                errors.append("phase %d: an un-captured group (%d x %d, seed %d) differs from the oracle after its own run" % (rep, g.mb, g.nb, g.seed))
        # other inputs under the other groups' feet: a replay that ran one of their work lists would now change their outputs
        for g in phase:
            g.fresh(next(seeds))
            g.upload(outputs=False)
        for c in cap_groups:
            c.fresh(5000 + 10 * rep + c.nb)
            c.upload()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        ok = True
        for c in cap_groups:
            if not same_bits(c.got(), c.oracle()):
                ok = False
                errors.append("replay %d: the captured group of %d invokes does not have the oracle's bits (%d of %d elements differ)" % (
                    rep, c.mb * c.nb, int((ed.bits(c.got()) != ed.bits(c.oracle())).sum()), c.C0.size))
        for g, w in zip(phase, want):
            if not same_bits(g.got(), w):
                ok = False
                errors.append("replay %d rewrote the output of an un-captured group (%d x %d, seed %d)" % (rep, g.mb, g.nb, g.seed))
        replays.append(ok)
        if rep == 0 and big_seen < NSEG:
            errors.append("fewer recorded groups than segments before the first replay: the captured segment was not evicted")
        if slot_flushes < SLOTS * (rep + 1):
            errors.append("phase %d: fewer slot-taking flushes than ring slots" % rep)
    # the un-captured run of the captured groups afterwards: the same bits once more (their segment, re-recorded or not)
    rt.set_stream(None)
    for c in cap_groups:
        c.fresh(9000 + c.nb)
        c.upload()
        run(c)
    rt.synchronize()
    for c in cap_groups:
        if not same_bits(c.got(), c.oracle()):
            errors.append("the un-captured run of a captured group after the replays differs from the oracle")
    stats = rt.tile_queue_stats()
    return {"scenario": "queue warm" if warm else "queue cold", "errors": errors, "replays": replays, "flushes": flushes, "slot_flushes": slot_flushes,
            "recorded_groups": big_seen, "in_capture": in_capture, "queue_stats": [b - a for a, b in zip(stats0, stats)], "groups_kept": len(keep)}


def small_split_scenario(rt):
    """the split of brgemm_bf16_small.hip lives in grouped launches: a tile-queue group of 6 bf16 32x32x32 invokes with 8 K steps each under
    a forced split count of 2. Captured, the group gathers into a pinned slot and launches unsplit; between the replays the same group runs
    un-captured and split on the same stream, into other outputs"""
    import torch
    errors = []
    rt.set_async(True)
    rt.set_tile_queue(1)
    h = rt.brgemm_dispatch(BF16, 32, 32, 32, 32, 32, 32, 1024, 1024, 4 | 2048)
    grp, twin = TileGroup(2, 3, 31, dt=BF16, kb=4), TileGroup(2, 3, 31, dt=BF16, kb=4)
    prev = rt.force_split(2)

    def step(g=grp):
        g.invoke(rt, h)
        rt.flush()
        return rt.last_grouped_kernel()

    try:
        graph, inside, s = captured(rt, step, warm=1)
        outside = []
        replays = []
        for rep in range(3):
            for g in (grp, twin):
                g.fresh(300 + rep)
                g.upload()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            try:
                rt.set_stream(s)
                outside.append(step(twin))
            finally:
                rt.set_stream(None)
            rt.synchronize()
            torch.cuda.synchronize()
            ref = grp.oracle()
            replays.append(same_bits(grp.got(), ref))
            if not replays[-1]:
                errors.append("replay %d does not have the oracle's bits" % rep)
            if not same_bits(twin.got(), ref):
                errors.append("the un-captured split group after replay %d does not have the oracle's bits" % rep)
    finally:
        rt.force_split(prev)
    return {"scenario": "small", "errors": errors, "replays": replays, "inside": inside, "outside": outside}


# ------------------------------------------------------------------------------------------------ the scratch block's edges
def split_call(rt, case, bn, P, bufs):
    """one skinny call under BN `bn` and P parts on the runtime's current stream, no synchronisation; the reported kernel"""
    rt.set_skinny_bf16(bn)
    rt.set_skinny_split(P)
    try:
        return invoke(rt, case, case.dispatch(rt), bufs)
    finally:
        rt.set_skinny_split(0)
        rt.set_skinny_bf16(0)


def growth_scenario(rt):
    import torch
    errors = []
    rt.set_async(True)
    bn = 64
    small = Case(2, 17, 200, 72, 1, 11, exact=True, beta0=True, bias=True, relu=True)
    large = Case(2, 17, 9 * 64 + 8, 64, 16, 12, exact=True, beta0=True, bias=True, relu=True)
    floats = [-(-c.n // bn) * min(P, c.br * -(-c.k // 32)) * 32 * bn for c, P in ((small, 3), (large, 16))]
    if not floats[0] <= 1 << 18 < floats[1] <= 8 << 20:
        errors.append("the cases do not straddle the first 1 MiB block: %r partial floats" % (floats,))
    seq = [(small, 3), (large, 16), (small, 3)]
    for c in (small, large):
        if not np.array_equal(c.oracle()[c.win], c.fp64()):
            errors.append("not an exact case")
    bufs = [c.device() for c, _ in seq]
    sbefore = rt.skinny_split_stats()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    kernels = []
    try:
        rt.set_stream(s)
        for (c, P), b in zip(seq, bufs):  # back to back: nothing waits between the launches
            kernels.append(split_call(rt, c, bn, P, b))
    finally:
        rt.set_stream(None)
    rt.synchronize()
    torch.cuda.synchronize()
    for i, ((c, P), b, kern) in enumerate(zip(seq, bufs, kernels)):
        if kern != split_text(c.image, c.m, bn):
            errors.append("call %d reported %r" % (i, kern))
        got, ref = download(b[2], c), c.oracle()
        if not same_bits(got[c.win], ref[c.win]):
            errors.append("call %d (n = %d, P = %d) does not have the oracle's bits" % (i, c.n, P))
        if not c.outside_untouched(got):
            errors.append("call %d wrote outside its window" % i)
    moved = rt.skinny_split_stats()[0] - sbefore[0]
    if moved != 3:
        errors.append("the split counter moved by %d" % moved)
    return {"scenario": "growth", "errors": errors, "kernels": kernels, "partial_floats": floats, "split_launches": moved}


def streams_scenario(rt):
    """(device, stream) pairs in the order split_scratch_for sees them: the default (null) stream is a pair like any other, so it is the
    first; seventeen side streams follow - the first fifteen are pairs 2 .. 16 and get a block, the sixteenth is the 17th pair and runs
    unsplit, and so does the seventeenth"""
    import torch
    errors = []
    rt.set_async(True)
    bn, P = 32, 3
    case = Case(4, 17, bn + 8, 72, 1, 21, exact=True, beta0=True, bias=True, relu=True)
    ref = case.oracle()
    if not np.array_equal(ref[case.win], case.fp64()):
        errors.append("not an exact case")
    streams = [None] + [torch.cuda.Stream() for _ in range(SPLIT_MAX_BLOCKS + 1)]
    handles = {0 if s is None else s.cuda_stream for s in streams}
    if len(handles) != len(streams):
        errors.append("the streams are not %d different ones: %d" % (len(streams), len(handles)))
    kernels, moved, unsplit_moved = [], [], []
    for i, s in enumerate(streams):
        bufs = case.device()
        torch.cuda.synchronize()
        sb, ub = rt.skinny_split_stats(), rt.skinny_bf16_stats()
        try:
            rt.set_stream(s)
            kernels.append(split_call(rt, case, bn, P, bufs))
        finally:
            rt.set_stream(None)
        rt.synchronize()
        torch.cuda.synchronize()
        sa, ua = rt.skinny_split_stats(), rt.skinny_bf16_stats()
        moved.append(sa[0] - sb[0])
        unsplit_moved.append(ua[0] - ub[0])
        took = i < SPLIT_MAX_BLOCKS
        want = split_text(case.image, case.m, bn) if took else skinny_text(case.image, case.m, bn)
        if kernels[-1] != want:
            errors.append("pair %d reported %r, not %r" % (i + 1, kernels[-1], want))
        if moved[-1] != (1 if took else 0) or (took and sa != expected_split_stats(sa[0], case.n, case.k, case.br, bn, P)):
            errors.append("pair %d: the split counter %r -> %r" % (i + 1, sb, sa))
        if unsplit_moved[-1] != 1:
            errors.append("pair %d: the skinny counter moved by %d" % (i + 1, unsplit_moved[-1]))
        got = download(bufs[2], case)
        if not same_bits(got[case.win], ref[case.win]) or not case.outside_untouched(got):
            errors.append("pair %d: not the oracle's bits, or wrote outside the window" % (i + 1))
    return {"scenario": "streams", "errors": errors, "kernels": kernels, "split_moved": moved, "skinny_moved": unsplit_moved}


if __name__ == "__main__":
    rt = pkg.get_runtime()
    what = sys.argv[1:]
    if what[:1] == ["queue"]:
        out = queue_scenario(rt, warm=what[1] == "warm")
    elif what == ["small"]:
        out = small_split_scenario(rt)
    elif what == ["growth"]:
        out = growth_scenario(rt)
    else:
        out = streams_scenario(rt)
    rt.synchronize()
    print(json.dumps(out))
