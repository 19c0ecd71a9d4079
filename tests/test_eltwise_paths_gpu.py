"""Every kernel instance and every loop of tpp-mlir_amd/csrc/eltwise.hip that a direct (non-queued) unary / binary invoke can reach,
bit for bit against the CPU oracle, through the C-ABI on device pointers - and for every case the kernel instance the launcher
reports (xsmm_hip_last_eltwise_kernel / _grid) is asserted, so a shape chosen for the 16-byte path cannot pass on the element path.

  a. SPAN GEOMETRY of unary_kernel / binary_kernel: a block owns one span of `per` packs (span_of_block); below 4 194 304 packs every
     lane handles exactly one pack, which is all the other files reach. Here the reported grid is turned into the set of things lanes
     do (span_classes) and every class is reached by every instance: <T,V> flat, <T,V> with the row division, <T,1>.
  b. VECTOR ELIGIBILITY: each single reason drops a case to <T,1>; a misaligned row- / scalar-broadcast operand does not.
  c. TRANSPOSES: multi-tile shapes on the 128 x 128 and the 64 x 64 instance (diagonal tile order) and on the ragged fallback.
  d. VNNI-2 PACK: both store policies around the 64 MiB switch, the grid-y limit, both generic kernels with a repeating loop.
  e. test_zz_coverage (runs last): the table INVENTORY is the list of kernel instances; every one must have been reached, in
     every class the table asks for, and a name the library reports that the table does not hold fails too.

Every case compares the WHOLE output buffer - window, row padding and a tail behind the window - with the oracle's; the buffer is
prefilled with a non-zero pattern on both sides. Moves (identity, transpose, pack) run on random bit patterns incl. NaN payloads;
bf16 NaNs are kept quiet, because the oracle's identity goes through an f32 (it would quiet a signalling NaN) while the kernel moves
the storage word. Arithmetic runs on finite values: magnitudes in [0.5, 2), random signs on the left operand (both operands of a
division positive), one IEEE operation and one rounding on both sides - bit-exact, division included (test_parity_gpu.py).

The direct-transpose rewrite (dt_defer, runtime.cpp) could remember a transpose instead of launching it: the module's runtime
fixture switches it off with set_fold_transpose(False), together with asynchronous mode and the tile queue, and restores all three.

The large inputs (about 270 MB per buffer) are generated once per dtype and stay on the device for the whole module; the oracle runs
on row blocks in a pool of threads (ctypes releases the GIL; rows are independent), as do the fills and comparisons. Peak device use is about 3 GiB.
"""
import importlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("tpp-mlir_amd")
F32, BF16 = 1, 2
TN = {F32: "f32", BF16: "bf16"}
VW = {F32: 4, BF16: 8}  # elements of a 16-byte pack
U_ID, U_ZERO, U_RELU, U_VNNI2, U_TRANS = 1, 2, 5, 28, 29
TAIL = 72  # elements behind the output window that are compared too
PAT = {F32: 0x7FC5A5A5, BF16: 0x7FD5}  # prefill of every output buffer (a NaN: no case computes it)
BIG_PACKS = (1 << 24) + (1 << 17)  # capacity of the large buffers, in 16-byte packs

THREADS = max(2, min(16, orc.usable_cpus()[0]))
POOL = ThreadPoolExecutor(THREADS)
REACHED = {}  # kernel instance name -> set of classes it was reached in ("" = at all)


# ---------------------------------------------------------------- geometry of a launch
BODY_ONLY, BODY_TAIL, TAIL1, TAIL2, TAIL3, MIXED, IDLE, RAGGED, REPEAT = (
    "body only", "body then tail", "tail x1", "tail x2", "tail x3", "partial span: some lanes body, some not", "blocks that own nothing",
    "total not a multiple of 256", "grid-stride loop repeats")
STREAM_CLASSES = {BODY_ONLY, BODY_TAIL, TAIL2, TAIL3, MIXED, IDLE, RAGGED}


def span_classes(total, grid):
    """what the lanes of a unary_kernel / binary_kernel launch of `grid` blocks over `total` packs do. The one formula is
    span_of_block's (eltwise.hip):
        const int64_t per = (((total + gridDim.x - 1) / gridDim.x) + 255) & ~(int64_t)255;
    block b owns [b * per, min((b + 1) * per, total)); lane t starts at b * per + t, runs the four-round body while
    idx + 3 * 256 < end (idx += 1024), then single rounds while idx < end (idx += 256)."""
    per = (((total + grid - 1) // grid) + 255) & ~255
    full, rem = divmod(total, per)
    assert full + (1 if rem else 0) <= grid, "the grid does not cover the index space"
    out = set()
    if total % 256:
        out.add(RAGGED)
    if full + (1 if rem else 0) < grid:
        out.add(IDLE)
    for length in ([per] if full else []) + ([rem] if rem else []):
        lanes = []
        for t in range(256):
            idx, body, tail = t, 0, 0
            while idx + 3 * 256 < length:
                body, idx = body + 1, idx + 1024
            while idx < length:
                tail, idx = tail + 1, idx + 256
            lanes.append((body, tail))
        bodies, tails = {b for b, _ in lanes}, {t for _, t in lanes}
        if min(bodies) >= 1 and tails == {0} and length == per == 1024:
            out.add(BODY_ONLY)
        elif min(bodies) >= 1 and min(tails) >= 1:
            out.add(BODY_TAIL)
        elif min(bodies) == 0 and max(bodies) >= 1:
            out.add(MIXED)
        elif bodies == {0} and tails in ({1}, {2}, {3}):
            out.add({1: TAIL1, 2: TAIL2, 3: TAIL3}[max(tails)])
    return out


def test_span_classes_helper():
    """the helper on the issue's own examples (no launch)"""
    assert span_classes(256 * 1000, 1000) == {TAIL1}
    assert span_classes(16384 * 256 + 1, 16384) == {TAIL2, IDLE, RAGGED}  # per = 512: about half the grid idle, a last span of one pack
    assert span_classes(16384 * 1024, 16384) == {BODY_ONLY}
    assert span_classes(16384 * 1280, 16384) == {BODY_TAIL}
    assert span_classes(16384 * 768, 16384) == {TAIL3}
    assert span_classes(16777734, 16384) == {BODY_TAIL, MIXED, IDLE, RAGGED}


def chunks(n):
    """[0, n) in pieces for the pool (numpy's fills and comparisons release the GIL too)"""
    step = max(1 << 20, -(-n // THREADS))
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def reached(name, classes=()):
    REACHED.setdefault(name, set()).update(classes)
    REACHED[name].add("")


# ---------------------------------------------------------------- buffers
class Arena:
    """host and device copies of the inputs of one dtype and one output buffer of the same size:
    bits (random words; bf16 NaNs quiet), A (signed, |x| in [0.5, 2)), B (positive, in [0.5, 2))"""

    def __init__(self, dt, packs, seed):
        import torch
        self.dt, self.n = dt, packs * VW[dt]
        rng = np.random.default_rng(seed)
        if dt == F32:
            bits = rng.integers(0, 1 << 32, self.n, dtype=np.uint32)
            self.A = ((bits & np.uint32(0x00FFFFFF)) + np.uint32(0x3F000000)) | (bits & np.uint32(0x80000000))
            self.B = ((bits >> np.uint32(7)) & np.uint32(0x00FFFFFF)) + np.uint32(0x3F000000)
        else:
            bits = rng.integers(0, 1 << 16, self.n, dtype=np.uint16)
            self.A = ((bits & np.uint16(0xFF)) + np.uint16(0x3F00)) | (bits & np.uint16(0x8000))
            self.B = ((bits >> np.uint16(7)) & np.uint16(0xFF)) + np.uint16(0x3F00)
            bits[(bits & np.uint16(0x7FFF)) > np.uint16(0x7F80)] |= np.uint16(0x40)
        self.bits = bits
        self.sdt = np.int32 if dt == F32 else np.int16
        self.host = {"bits": self.bits, "A": self.A, "B": self.B}
        self.dev = {k: torch.from_numpy(v.view(self.sdt)).cuda() for k, v in self.host.items()}
        self.ref = np.empty(self.n, dtype=bits.dtype)
        self.dO = torch.empty(self.n, dtype=self.dev["A"].dtype, device="cuda")
        self.land = torch.empty(self.n, dtype=self.dO.dtype, pin_memory=True)
        self.got = self.land.numpy().view(bits.dtype)
        self.pat = int(np.array([PAT[dt]], dtype=bits.dtype).view(self.sdt)[0])

    def start(self, span, inplace=None):
        """both output buffers prefilled (with the pattern, or with the operand an in-place case overwrites)"""
        import torch
        assert span <= self.n, "case larger than the arena"
        if inplace is None:
            list(POOL.map(lambda c: self.ref[c[0]:c[1]].fill(PAT[self.dt]), chunks(span)))
            self.dO[:span].fill_(self.pat)
        else:
            list(POOL.map(lambda c: np.copyto(self.ref[c[0]:c[1]], self.host[inplace][c[0]:c[1]]), chunks(span)))
            self.dO[:span].copy_(self.dev[inplace][:span])
        torch.cuda.synchronize()

    def check(self, span, what):
        import torch
        self.land[:span].copy_(self.dO[:span])
        torch.cuda.synchronize()
        got, ref = self.got[:span], self.ref[:span]
        if not all(POOL.map(lambda c: np.array_equal(got[c[0]:c[1]], ref[c[0]:c[1]]), chunks(span))):
            bad = np.flatnonzero(got != ref)
            cut = np.flatnonzero(np.diff(bad) != 1)
            runs = list(zip(bad[np.r_[0, cut + 1]].tolist(), (np.diff(np.r_[0, cut + 1, bad.size])).tolist()))
            again = self.dO[:span].cpu().numpy().view(ref.dtype)  # a second read of the device buffer: the kernel's result, or the transfer?
            raise AssertionError("%s: %d of %d words differ from the oracle, first at %d (got %#x, want %#x); %d runs (start, length), the first %s; "
                                 "a second read of the device buffer differs from the oracle in %d words and from the first read in %d" % (
                                     what, bad.size, span, int(bad[0]), int(got[bad[0]]), int(ref[bad[0]]), len(runs), runs[:12],
                                     int((again != ref).sum()), int((again != got).sum())))


_ARENAS = {}


def arena(dt, big):
    key = (dt, big)
    if key not in _ARENAS:
        _ARENAS[key] = Arena(dt, BIG_PACKS if big else 1 << 16, 77 + dt + 10 * big)
    return _ARENAS[key]


@pytest.fixture(scope="module")
def rt():
    import torch
    r = pkg.get_runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    prev_async, prev_queue, prev_fold = r.set_async(False), r.set_tile_queue(0), r.set_fold_transpose(False)
    yield r
    r.synchronize()
    r.set_fold_transpose(prev_fold)
    r.set_tile_queue(prev_queue)
    r.set_async(prev_async)
    _ARENAS.clear()  # the large buffers go with the module
    torch.cuda.empty_cache()


def blocks(m, step=1):
    """row blocks for the oracle's threads (multiples of `step` rows)"""
    parts = THREADS if m >= 64 else 1
    per = -(-m // parts)
    per += -per % step
    return [(r0, min(per, m - r0)) for r0 in range(0, m, per)]


def in_extent(mode, m, n, ld):
    """elements of an operand that an m x n invoke reads"""
    return {"none": (m - 1) * ld + n, "row": (m - 1) * ld + 1, "col": n, "scalar": 1}[mode]


def in_off(mode, r0, ld):
    """element offset of row block r0 in an operand: none / row broadcast advance by rows, column / scalar broadcast do not"""
    return r0 * ld if mode in ("none", "row") else 0


U_FLAG = {"none": 0, "row": 2, "col": 4, "scalar": 8}
U_MODE = {v: k for k, v in U_FLAG.items()}


def run_unary(rt, ar, kind, m, n, ldi, ldo, flags=0, src="A", off_in=0, off_out=0, scalar=None, inplace=False, expect=None):
    """one unary invoke on the arena's device buffers against the oracle on its host buffers; returns (kernel name, grid)"""
    dt = ar.dt
    if kind == U_TRANS:
        span = off_out + (n - 1) * ldo + m + TAIL
    elif kind == U_VNNI2:
        span = off_out + (m // 2 - 1) * 2 * ldo + 2 * n + TAIL
    else:
        span = off_out + (m - 1) * ldo + n + TAIL
    ar.start(span, src if inplace else None)
    X, dX = (ar.ref, ar.dO) if inplace else (ar.host[src], ar.dev[src])
    mode = U_MODE[flags]
    assert inplace or scalar is not None or off_in + in_extent(mode, m, n, ldi) <= ar.n, "input larger than the arena"

    def oracle(blk):
        r0, rr = blk
        if kind == U_TRANS:
            orc.unary(kind, dt, rr, n, ldi, ldo, flags, X, off_in + r0 * ldi, ar.ref, off_out + r0)
        elif kind == U_VNNI2:
            orc.unary(kind, dt, rr, n, ldi, ldo, flags, X, off_in + r0 * ldi, ar.ref, off_out + (r0 // 2) * 2 * ldo)
        elif scalar is not None:
            orc.unary_scalar(kind, dt, rr, n, ldi, ldo, flags, scalar, ar.ref, off_out + r0 * ldo)
        else:
            orc.unary(kind, dt, rr, n, ldi, ldo, flags, X, off_in + in_off(mode, r0, ldi), ar.ref, off_out + r0 * ldo)
    list(POOL.map(oracle, blocks(m, 2 if kind == U_VNNI2 else 1)))
    h = rt.unary_dispatch(kind, dt, m, n, ldi, ldo, flags)
    if scalar is not None:
        rt.unary_scalar(dt, h, scalar, ar.dO, off_out)
    else:
        rt.unary(dt, h, dX, off_in, ar.dO, off_out)
    rt.synchronize()
    name, grid = rt.last_eltwise_kernel(), rt.last_eltwise_grid()
    what = "unary kind %d %s %d x %d ldi %d ldo %d flags %d offsets %d/%d%s%s [%s, %d blocks]" % (
        kind, TN[dt], m, n, ldi, ldo, flags, off_in, off_out, " scalar invoke" if scalar is not None else "",
        " in place" if inplace else "", name, grid)
    if expect is not None:
        assert name == expect, what + ": expected " + expect
    ar.check(span, what)
    return name, grid


B_BITS = {"none": (0, 0), "row": (1, 2), "col": (4, 8), "scalar": (16, 32)}


def run_binary(rt, ar, kind, m, n, ldl, ldr, ldo, lmode="none", rmode="none", lsrc="A", rsrc="B", off_l=0, off_r=0, off_out=0,
               inplace=False, expect=None):
    """one binary invoke (inplace: out == lhs); returns (kernel name, grid)"""
    dt = ar.dt
    flags = B_BITS[lmode][0] | B_BITS[rmode][1]
    span = off_out + (m - 1) * ldo + n + TAIL
    ar.start(span, lsrc if inplace else None)
    L, dL = (ar.ref, ar.dO) if inplace else (ar.host[lsrc], ar.dev[lsrc])
    R, dR = ar.host[rsrc], ar.dev[rsrc]
    assert off_l + in_extent(lmode, m, n, ldl) <= ar.n and off_r + in_extent(rmode, m, n, ldr) <= ar.n, "input larger than the arena"

    def oracle(blk):
        r0, rr = blk
        orc.binary(kind, dt, rr, n, ldl, ldr, ldo, flags, L, off_l + in_off(lmode, r0, ldl), R, off_r + in_off(rmode, r0, ldr),
                   ar.ref, off_out + r0 * ldo)
    list(POOL.map(oracle, blocks(m)))
    h = rt.binary_dispatch(kind, dt, m, n, ldl, ldr, ldo, flags)
    rt.binary(dt, h, dL, off_l, dR, off_r, ar.dO, off_out)
    rt.synchronize()
    name, grid = rt.last_eltwise_kernel(), rt.last_eltwise_grid()
    what = "binary kind %d %s %d x %d ldl %d ldr %d ldo %d lhs %s rhs %s offsets %d/%d/%d%s [%s, %d blocks]" % (
        kind, TN[dt], m, n, ldl, ldr, ldo, lmode, rmode, off_l, off_r, off_out, " out == lhs" if inplace else "", name, grid)
    if expect is not None:
        assert name == expect, what + ": expected " + expect
    ar.check(span, what)
    return name, grid


def uname(dt, vec, flat=False):
    return "unary_kernel<%s,v%d>%s" % (TN[dt], VW[dt] if vec else 1, ", flat" if flat else "")


def bname(dt, vec, flat=False):
    return "binary_kernel<%s,v%d>%s" % (TN[dt], VW[dt] if vec else 1, ", flat" if flat else "")


def packs_of(name, dt, m, n):
    return m * n if ",v1>" in name else m * (n // VW[dt])


# ---------------------------------------------------------------- a. span geometry
# (rows, packs per row) whose product reaches the class set on the right; the narrow forms have one / two packs per row
G_BODY = (4096, 4096)          # 2^24 packs: per = 1024, every span full
G_BODY_TAIL = (3989, 4206)     # 16 777 734: per = 1280, 13 107 full spans, a last span of 774 packs (lanes 0 .. 5 run the body), idle blocks
G_TAIL2 = (2049, 2049)         # 4 198 401: per = 512
G_TAIL3 = (3000, 3000)         # 9 000 000: per = 768
G_TAIL2_NARROW = (4198401, 1)
G_TAIL3_NARROW = (4500000, 2)
WANT = {G_BODY: {BODY_ONLY}, G_BODY_TAIL: {BODY_TAIL, MIXED, IDLE, RAGGED}, G_TAIL2: {TAIL2, IDLE, RAGGED}, G_TAIL3: {TAIL3, IDLE, RAGGED},
        G_TAIL2_NARROW: {TAIL2, IDLE, RAGGED}, G_TAIL3_NARROW: {TAIL3, IDLE, RAGGED}}


def geometry_case(rt, ar, family, form, geom, i):
    """one launch of unary_kernel / binary_kernel (`family`) in the flat, the strided (row division) or the element (`v1`) form over the
    pack grid `geom`; the class set is computed from the REPORTED grid and must hold the set the shape was chosen for"""
    dt, V = ar.dt, VW[ar.dt]
    m, nv = geom
    if form == "v1":
        # the same numbers as ELEMENTS; each launch leaves the 16-byte path for another single reason
        n = nv
        reason = ("out+1", "n", "n", "ldo")[i] if n % V else ("out+1", "ldo")[i % 2]
        assert reason != "n" or n % V
        ldo = n + (1 if reason == "ldo" else 0 if i % 2 == 0 else V)
        ldi, off_out = (n if ldo == n else n + 2 * V), (1 if reason == "out+1" else 0)
        expect = (uname if family == "unary" else bname)(dt, False)
    else:
        n = nv * V
        ldo = n if form == "flat" else n + V
        ldi = n if form == "flat" else n + (2 * V if nv > 2 else V)
        off_out = 0 if form == "flat" else 2 * V
        expect = (uname if family == "unary" else bname)(dt, True, form == "flat")
    if family == "unary":
        kind, src = ((U_RELU, "A"), (U_ID, "bits"))[i % 2]
        name, grid = run_unary(rt, ar, kind, m, n, ldi, ldo, 0, src, V, off_out, expect=expect)
    else:
        kind = (1, 3, 2, 4)[i % 4]
        name, grid = run_binary(rt, ar, kind, m, n, ldi, ldo if form == "flat" else n + (3 * V if nv > 2 else V), ldo, lsrc="B" if kind == 4 else "A",
                                off_l=V, off_r=2 * V, off_out=off_out, expect=expect)
    got = span_classes(packs_of(name, dt, m, n), grid)
    assert WANT[geom] <= got, "%s over %d x %d: lanes do %s, the shape was chosen for %s" % (name, m, nv, sorted(got), sorted(WANT[geom]))
    reached(name, got)


@pytest.mark.parametrize("form", ["flat", "strided", "v1"])
@pytest.mark.parametrize("family", ["unary", "binary"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_span_geometry(rt, dt, family, form):
    """every class of span_classes on every streaming instance, classes asserted from the reported grid. The strided form (ldo > n,
    ldi > n: the row division runs, 32-bit) also runs rows of one and of two packs, millions of them"""
    ar = arena(dt, True)
    geoms = [G_BODY, G_BODY_TAIL, G_TAIL2, G_TAIL3]
    if form == "strided":
        geoms[2:] = [G_TAIL2_NARROW, G_TAIL3_NARROW]
    for i, geom in enumerate(geoms):
        geometry_case(rt, ar, family, form, geom, i)


@pytest.mark.parametrize("vec", [True, False], ids=["v16B", "v1"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_unary_ops_on_body_then_tail(rt, dt, vec):
    """identity, relu, zero and the scalar invoke, every broadcast mode and relu in place on the body-then-tail shape"""
    ar, V = arena(dt, True), VW[dt]
    m, nv = G_BODY_TAIL
    n = nv * V if vec else nv  # (4206 is no multiple of 4: the element form by n % V)
    for kind, src in ((U_ID, "bits"), (U_RELU, "A"), (U_ZERO, "A")):
        name, grid = run_unary(rt, ar, kind, m, n, n, n, 0, src, V, 0, expect=uname(dt, vec, vec))
        assert BODY_TAIL in span_classes(packs_of(name, dt, m, n), grid)
    # (the op x broadcast matrix is complete on the element form, whose buffers are V times smaller; the 16-byte form runs every op
    # and every broadcast mode once - the pairs left out there differ from a pair that runs in the op's arithmetic only)
    for kind, val in ((U_ID, 1.2345678), (U_RELU, -3.0), (U_RELU, 0.75), (U_ZERO, 9.0))[:2 if vec else 4]:
        run_unary(rt, ar, kind, m, n, 1, n, 8, scalar=val, expect=uname(dt, vec, vec))
    for kind, src, modes in ((U_ID, "bits", "rs" if vec else "rcs"), (U_RELU, "A", "c" if vec else "rcs")):
        # row / column broadcasts keep the row division; a scalar read from memory is contiguous (flat); none of the three needs an
        # aligned or V-strided input - except the column broadcast, whose 16-byte loads need the pointer (offset V)
        if "r" in modes:
            run_unary(rt, ar, kind, m, n, 1, n, 2, src, 3, 0, expect=uname(dt, vec))
        if "c" in modes:
            run_unary(rt, ar, kind, m, n, n, n + (V if vec else 0), 4, src, V, 0, expect=uname(dt, vec))
        if "s" in modes:
            run_unary(rt, ar, kind, m, n, 1, n, 8, src, 5, 0, expect=uname(dt, vec, vec))
    run_unary(rt, ar, U_RELU, m, n, n, n, 0, "A", 0, 0, inplace=True, expect=uname(dt, vec, vec))
    if not vec:
        run_unary(rt, ar, U_RELU, m, n, n + 1, n + 1, 0, "A", 1, 1, inplace=True, expect=uname(dt, vec))


@pytest.mark.parametrize("vec", [True, False], ids=["v16B", "v1"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_binary_ops_on_body_then_tail(rt, dt, vec):
    """add, mul, sub, div, every broadcast mode of each operand and out == lhs on the body-then-tail shape"""
    ar, V = arena(dt, True), VW[dt]
    m, nv = G_BODY_TAIL
    n = nv * V if vec else nv
    for kind in (1, 2, 3, 4):
        name, grid = run_binary(rt, ar, kind, m, n, n, n, n, lsrc="B" if kind == 4 else "A", off_l=V, off_r=2 * V, expect=bname(dt, vec, vec))
        assert BODY_TAIL in span_classes(packs_of(name, dt, m, n), grid)
    for j, mode in enumerate(("row", "col", "scalar")):
        ld = n if mode == "col" else 1
        off = V if mode == "col" else 3  # (a column broadcast is read with 16-byte loads; a row / scalar one element by element)
        flat = vec and mode == "scalar"
        run_binary(rt, ar, (3, 4, 1)[j], m, n, ld, n, n, lmode=mode, lsrc="B", off_l=off, off_r=V, expect=bname(dt, vec, flat))
        run_binary(rt, ar, (4, 2, 3)[j], m, n, n, ld, n, rmode=mode, lsrc="B", off_l=V, off_r=off, expect=bname(dt, vec, flat))
    run_binary(rt, ar, 1, m, n, n, n, n, inplace=True, off_r=V, expect=bname(dt, vec, vec))
    if not vec:
        run_binary(rt, ar, 2, m, n, n, n, n, rmode="col", inplace=True, off_r=V, expect=bname(dt, vec))


# ---------------------------------------------------------------- b. vector eligibility
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_unary_vector_eligibility(rt, dt):
    """each single reason alone drops a unary case to the element kernel; a misaligned row / scalar broadcast operand does not"""
    ar, V = arena(dt, False), VW[dt]
    m, n = 24, 6 * V
    vec, vec_flat, v1 = uname(dt, True), uname(dt, True, True), uname(dt, False)
    cases = [
        # (ldi, ldo, flags, off_in, off_out, expect)
        (n, n, 0, V, 0, vec_flat),
        (n + V, n + 2 * V, 0, V, 2 * V, vec),
        (n + 1, n + 1, 0, V, 0, None),                # n % V (by n below)
        (n + V, n + V + 1, 0, V, 0, v1),              # ldo % V
        (n + V + 1, n + V, 0, V, 0, v1),              # ldi % V, no broadcast
        (n + V, n + V, 0, V, 1, v1),                  # output off 16 bytes
        (n + V, n + V, 0, 1, 0, v1),                  # input off 16 bytes, no broadcast
        (n, n + V, 4, 1, 0, v1),                      # input off 16 bytes, column broadcast
        (n, n + V, 4, V, 0, vec),                     # column broadcast, aligned
        (1, n + V, 2, 3, 0, vec),                     # row broadcast, misaligned: stays on the 16-byte path
        (1, n, 8, 3, 0, vec_flat),                    # scalar broadcast, misaligned: stays, and flat
        (7, n + V, 2, 1, 0, vec),                     # row broadcast with an odd stride
    ]
    for kind, src in ((U_ID, "bits"), (U_RELU, "A")):
        for ldi, ldo, flags, off_in, off_out, expect in cases:
            if expect is None:
                name, _ = run_unary(rt, ar, kind, m, n + 1, ldi, ldo, flags, src, off_in, off_out, expect=v1)
            else:
                name, _ = run_unary(rt, ar, kind, m, n, ldi, ldo, flags, src, off_in, off_out, expect=expect)
            reached(name)
    # zero and the scalar invoke read nothing: only n, ldo and the output pointer count
    for kind, val in ((U_ZERO, None), (U_ID, 2.5)):
        for ldi, ldo, off_out, n_, expect in ((n + 1, n, 0, n, vec_flat), (n + 1, n + V, 0, n, vec), (n, n + 1, 0, n, v1), (n, n + V, 1, n, v1),
                                              (n, n + 1, 0, n + 1, v1)):
            if val is None:
                run_unary(rt, ar, kind, m, n_, ldi, ldo, 0, "A", 1, off_out, expect=expect)
            else:
                run_unary(rt, ar, kind, m, n_, ldi, ldo, 8, off_out=off_out, scalar=val, expect=expect)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_binary_vector_eligibility(rt, dt):
    """the same for each operand of a binary"""
    ar, V = arena(dt, False), VW[dt]
    m, n = 24, 6 * V
    vec, vec_flat, v1 = bname(dt, True), bname(dt, True, True), bname(dt, False)
    P = n + V
    cases = [
        # (n, ldl, ldr, ldo, lmode, rmode, off_l, off_r, off_out, expect)
        (n, n, n, n, "none", "none", V, 2 * V, 0, vec_flat),
        (n, P, P + V, P, "none", "none", V, 2 * V, V, vec),
        (n + 1, P, P, P, "none", "none", V, V, 0, v1),           # n % V
        (n, P, P, P + 1, "none", "none", V, V, 0, v1),           # ldo % V
        (n, P + 1, P, P, "none", "none", V, V, 0, v1),           # ldl % V
        (n, P, P + 1, P, "none", "none", V, V, 0, v1),           # ldr % V
        (n, P, P, P, "none", "none", V, V, 1, v1),               # output off 16 bytes
        (n, P, P, P, "none", "none", 1, V, 0, v1),               # lhs off 16 bytes
        (n, P, P, P, "none", "none", V, 1, 0, v1),               # rhs off 16 bytes
        (n, n, P, P, "col", "none", 1, V, 0, v1),                # lhs column broadcast off 16 bytes
        (n, P, n, P, "none", "col", V, 1, 0, v1),                # rhs column broadcast off 16 bytes
        (n, n, P, P, "col", "none", V, V, 0, vec),
        (n, 1, P, P, "row", "none", 3, V, 0, vec),               # misaligned row broadcast: stays
        (n, P, 7, P, "none", "row", V, 1, 0, vec),
        (n, 1, n, n, "scalar", "none", 3, V, 0, vec_flat),       # misaligned scalar broadcast: stays, and flat
        (n, n, 1, n, "none", "scalar", V, 5, 0, vec_flat),
        (n, 1, 1, n, "scalar", "scalar", 3, 5, 0, vec_flat),
    ]
    for kind in (1, 4):
        for n_, ldl, ldr, ldo, lmode, rmode, off_l, off_r, off_out, expect in cases:
            name, _ = run_binary(rt, ar, kind, m, n_, ldl, ldr, ldo, lmode, rmode, "B", "B", off_l, off_r, off_out, expect=expect)
            reached(name)


# ---------------------------------------------------------------- c. transposes
def tname(dt, tile):
    return "transpose<%s>" % TN[dt] if tile is None else "transpose_vec<%s,%dx%d>" % (TN[dt], tile, tile)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_transpose_paths(rt, dt):
    """multi-tile transposes on each instance, ldi > n, ldo > m, offsets that keep 16-byte alignment where the vector kernels are meant;
    the fallback by each single reason on a shape the 128 x 128 instance would take"""
    ar, V = arena(dt, False), VW[dt]
    cases = []
    for m, n in ((384, 128), (128, 384), (256, 640), (384, 256)):      # tiles_n = 1; one tile row; tiles_n > tiles_m; tiles_n < tiles_m
        cases.append((m, n, n + V, m + 2 * V, V, 2 * V, 128))
    for m, n in ((192, 320), (128, 192), (64, 448), (448, 64), (320, 192), (192, 128)):
        cases.append((m, n, n + 2 * V, m + V, 2 * V, V, 64))
    m, n = 256, 384
    cases += [
        (m - 6, n, n + V, m + 2 * V, V, 2 * V, None),       # m % 64
        (m, n - 4, n + V, m + 2 * V, V, 2 * V, None),       # n % 64
        (m, n, n + V + 1, m + 2 * V, V, 2 * V, None),       # ldi % V
        (m, n, n + V, m + 2 * V + 1, V, 2 * V, None),       # ldo % V
        (m, n, n + V, m + 2 * V, 1, 2 * V, None),           # input off 16 bytes
        (m, n, n + V, m + 2 * V, V, 1, None),               # output off 16 bytes
        (m + 1, n + 1, n + 1, m + 1, 0, 0, None),
    ]
    for m, n, ldi, ldo, off_in, off_out, tile in cases:
        name, grid = run_unary(rt, ar, U_TRANS, m, n, ldi, ldo, 0, "bits", off_in, off_out, expect=tname(dt, tile))
        t = tile or 64
        assert grid == -(-m // t) * -(-n // t) and (grid > 1), (name, grid)
        reached(name)


# ---------------------------------------------------------------- d. VNNI-2 pack
def vnni_case(rt, m, n, ldi, ldo, expect, off_in=0, off_out=0, big=True):
    ar = arena(BF16, big)
    name, grid = run_unary(rt, ar, U_VNNI2, m, n, ldi, ldo, 0, "bits", off_in, off_out, expect=expect)
    # unpack property: out[(i / 2)][j][i % 2] read back in (i, j) order is the input
    out = ar.got[off_out: off_out + (m // 2) * 2 * ldo - 2 * (ldo - n)]
    src = ar.bits[off_in: off_in + m * ldi - (ldi - n)]
    for r0, rr in ((0, min(m, 64)), (m // 2 & ~1, min(m - (m // 2 & ~1), 64)), (m - 2, 2)):
        o = np.lib.stride_tricks.as_strided(out[(r0 // 2) * 2 * ldo:], (rr // 2, n, 2), (4 * ldo, 4, 2))
        s = np.lib.stride_tricks.as_strided(src[r0 * ldi:], (rr, n), (2 * ldi, 2))
        assert np.array_equal(o.transpose(0, 2, 1).reshape(rr, n), s), "unpack property, rows %d .." % r0
    if m * n <= 1 << 22:  # (the whole matrix where that is cheap)
        o = np.lib.stride_tricks.as_strided(out, (m // 2, n, 2), (4 * ldo, 4, 2))
        s = np.lib.stride_tricks.as_strided(src, (m, n), (2 * ldi, 2))
        assert np.array_equal(o.transpose(0, 2, 1).reshape(m, n), s), "unpack property"
    return name, grid


def test_vnni2_rows4_policies_around_64mib(rt):
    """write-through up to 64 MiB moved (m * n <= 16 777 216), plain stores beyond"""
    for m, n, ldi, ldo, expect in ((4096, 4096, 4096, 4096, "vnni2_rows4<wt>"), (4094, 4096, 4104, 4100, "vnni2_rows4<wt>"),
                                   (4098, 4096, 4104, 4100, "vnni2_rows4<plain>"), (4096, 4104, 4104, 4104, "vnni2_rows4<plain>"),
                                   (64, 48, 56, 52, "vnni2_rows4<wt>")):
        assert (m * n <= 1 << 24) == expect.endswith("<wt>")
        name, grid = vnni_case(rt, m, n, ldi, ldo, expect, 8, 16)
        assert grid == -(-(n // 4) // 256) * (m // 2)
        reached(name)


def test_vnni2_grid_y_limit(rt):
    """m / 2 = 65535 row pairs still fit the grid's y dimension; 65536 run on the generic 16-byte kernel"""
    for m, expect in ((131070, "vnni2_rows4<wt>"), (131072, "vnni2<v8>")):
        name, grid = vnni_case(rt, m, 72, 80, 76, expect, 8, 8)
        reached(name)
    assert grid == (65536 * 9 + 255) // 256


def test_vnni2_generic_loops_repeat(rt):
    """more pieces than 16384 x 256 lanes: the grid-stride loops of vnni2_kernel<8> and vnni2_kernel<1> take a second iteration"""
    for m, n, ldi, ldo, expect in ((131072, 528, 536, 532, "vnni2<v8>"), (4098, 2052, 2056, 2052, "vnni2<v1>")):
        name, grid = vnni_case(rt, m, n, ldi, ldo, expect, 8, 8)
        pieces = (m // 2) * (n // 8 if expect == "vnni2<v8>" else n)
        assert grid == 16384 and 256 * grid < pieces < 2 * 256 * grid, (name, grid, pieces)
        reached(name, {REPEAT})


def test_vnni2_element_path_by_each_reason(rt):
    m, n = 66, 48
    for ldi, ldo, off_in, off_out, n_ in ((56, 52, 8, 8, n - 4),    # n % 8
                                          (52, 52, 8, 8, n),        # ldi % 8
                                          (56, 50, 8, 8, n),        # ldo % 4
                                          (56, 52, 4, 8, n),        # input off 16 bytes
                                          (56, 52, 8, 4, n)):       # output off 16 bytes
        name, _ = vnni_case(rt, m, n_, ldi, ldo, "vnni2<v1>", off_in, off_out, big=False)
        reached(name)


# ---------------------------------------------------------------- e. coverage
INVENTORY = {}
for _t, _v in (("f32", 4), ("bf16", 8)):
    for _k in ("unary_kernel", "binary_kernel"):
        INVENTORY["%s<%s,v%d>, flat" % (_k, _t, _v)] = STREAM_CLASSES
        INVENTORY["%s<%s,v%d>" % (_k, _t, _v)] = STREAM_CLASSES
        INVENTORY["%s<%s,v1>" % (_k, _t)] = STREAM_CLASSES
    INVENTORY["transpose_vec<%s,128x128>" % _t] = set()
    INVENTORY["transpose_vec<%s,64x64>" % _t] = set()
    INVENTORY["transpose<%s>" % _t] = set()
INVENTORY.update({"vnni2_rows4<wt>": set(), "vnni2_rows4<plain>": set(), "vnni2<v8>": {REPEAT}, "vnni2<v1>": {REPEAT}})


def test_zz_coverage():
    """runs last: every kernel instance a direct element-wise launch can report was reached by the cases above, the streaming
    kernels in every class of span_classes; a reported name outside the table fails"""
    for name in sorted(REACHED):
        print("[eltwise paths] %-34s %s" % (name, "; ".join(sorted(REACHED[name] - {""})) or "reached"))
    unknown = set(REACHED) - set(INVENTORY)
    assert not unknown, "kernel names the table does not hold: %s" % sorted(unknown)
    missing = ["%s: %s" % (k, "; ".join(sorted(v - REACHED.get(k, set()))) or "not reached") for k, v in sorted(INVENTORY.items())
               if k not in REACHED or v - REACHED[k]]
    assert not missing, "not reached:\n  " + "\n  ".join(missing)
