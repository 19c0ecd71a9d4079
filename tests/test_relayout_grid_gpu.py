"""RELAYOUT GRIDS (tpp-mlir_amd/csrc/rt_relayout.h, relayout.hip): a replayed tile-queue group of per-block identity / VNNI-2 unary
invokes - a tensor.pack / unpack as the compiler lowers it (LowerPacksAndUnpacks.cpp:45-49,112-121) - runs as ONE launch over a
table of affine block runs. The result must be the same BITS the items write one by one: raw words moved, NaN payloads, -0 and
subnormals included, nothing outside the destination blocks touched - with the switch on or off, with the queue off, and in strict
mode. Groups that are not such grids stay on the item kernel."""
import importlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
pkg = importlib.import_module("tpp-mlir_amd")
F32, BF16 = 1, 2
IDENTITY, VNNI2 = 1, 28
GUARD = 64  # elements of poison in front of and behind every buffer
T = 32


def raw_bits(rng, n, dt):
    """random bit patterns with the awkward ones planted: NaN payloads, -0, subnormals, infinities"""
    if dt == F32:
        a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        special = [0x80000000, 0x00000001, 0x807fffff, 0x7fa00001, 0xffc12345, 0x7f800000, 0xff800000, 0x00400000]
    else:
        a = rng.integers(0, 2 ** 16, n, dtype=np.uint32).astype(np.uint16)
        special = [0x8000, 0x0001, 0x807f, 0x7fa1, 0xffc3, 0x7f80, 0xff80, 0x0040]
    idx = rng.choice(n, min(n, 64 * len(special)), replace=False)
    for i, j in enumerate(idx):
        a[j] = special[i % len(special)]
    return a


def poison(n, dt):
    return np.full(n, 0x7fc0dead if dt == F32 else 0x7fc1, np.uint32 if dt == F32 else np.uint16)


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int16).copy()).cuda()


def to_host(t, dt):
    return t.cpu().numpy().view(np.uint32 if dt == F32 else np.uint16)


def np_unary(kind, m, n, ldi, ldo, src, oi, dst, oo):
    """xsmm_unary_invoke's identity / VNNI-2 on raw words (numpy's relayout of the same bits)"""
    s = np.lib.stride_tricks.as_strided(src[oi:], shape=(m, n), strides=(ldi * src.itemsize, src.itemsize))
    if kind == IDENTITY:
        d = np.lib.stride_tricks.as_strided(dst[oo:], shape=(m, n), strides=(ldo * dst.itemsize, dst.itemsize))
        d[...] = s
    else:
        d = np.lib.stride_tricks.as_strided(dst[oo:], shape=(m // 2, n, 2), strides=(2 * ldo * dst.itemsize, 2 * dst.itemsize, dst.itemsize))
        d[...] = s.reshape(m // 2, 2, n).transpose(0, 2, 1)


# ---- call patterns: (handle tuple, [(src index, off_in, off_out)], source sizes, destination size); offsets without the guard ----
def pack(R, Cc, bm=T, bn=T, perm=False, ldo=None, out_block=None):
    """[R][Cc] -> blocks [R/bm][Cc/bn][bm][bn] (perm: [Cc/bn][R/bm], tools/tpp_replay --script pack_b's outer_dims_perm)"""
    ldo = bn if ldo is None else ldo
    out_block = bm * ldo if out_block is None else out_block
    RB, CB = R // bm, Cc // bn
    items = []
    for i in range(RB):
        for j in range(CB):
            ob = j * RB + i if perm else i * CB + j
            items.append((0, i * bm * Cc + j * bn, ob * out_block))
    return items, RB * CB * out_block, (bm, bn, Cc, ldo)


def unpack(R, Cc, bm=T, bn=T):
    RB, CB = R // bm, Cc // bn
    items = [(0, (i * CB + j) * bm * bn, i * bm * Cc + j * bn) for i in range(RB) for j in range(CB)]
    return items, R * Cc, (bm, bn, bn, Cc)


def run(rt, kind, dt, shape, flags, items, srcs, nout, passes=3, threads=1, base_shift=0):
    """the items `passes` times through the current queue mode into a poisoned, guard-banded destination; returns its bits and the
    relayout-grid stats / kernel text seen after every pass"""
    m, n, ldi, ldo = shape
    h = rt.unary_dispatch(kind, dt, m, n, ldi, ldo, flags)
    dsrc = [to_dev(s) for s in srcs]
    dout = to_dev(poison(nout + 2 * GUARD + base_shift, dt))
    seen = []

    def issue(part):
        for s, oi, oo in part:
            rt.unary(dt, h, dsrc[s], GUARD + base_shift + oi, dout, GUARD + base_shift + oo)

    for _ in range(passes):
        if threads == 1:
            issue(items)
        else:
            ws = [threading.Thread(target=issue, args=(items[t::threads],)) for t in range(threads)]
            for w in ws:
                w.start()
            for w in ws:
                w.join()
        rt.synchronize()
        seen.append((rt.relayout_grid_stats(), rt.last_grouped_kernel()))
    return to_host(dout, dt), seen


def reference(kind, dt, shape, items, srcs, nout, base_shift=0):
    m, n, ldi, ldo = shape
    out = poison(nout + 2 * GUARD + base_shift, dt)
    for s, oi, oo in items:
        np_unary(kind, m, n, ldi, ldo, srcs[s], GUARD + base_shift + oi, out, GUARD + base_shift + oo)
    return out


def sources(rng, dt, sizes, base_shift=0):
    out = []
    for sz in sizes:
        a = poison(sz + 2 * GUARD + base_shift, dt)
        a[GUARD + base_shift:GUARD + base_shift + sz] = raw_bits(rng, sz, dt)
        out.append(a)
    return out


@pytest.fixture
def rtq():
    rt = pkg.get_runtime()
    assert rt.device_count() >= 1
    prev_async = rt.set_async(True)
    prev_q = rt.set_tile_queue(1)
    prev_g = rt.set_relayout_grid(True)
    yield rt
    rt.synchronize()
    rt.set_relayout_grid(prev_g)
    rt.set_tile_queue(prev_q)
    rt.set_async(prev_async)


def assert_grid_from_second_pass(seen, n_items, runs=None):
    for p in range(1, len(seen)):
        (l0, i0), _ = seen[p - 1]
        (l1, i1), text = seen[p]
        assert text.startswith("relayout grid"), (p, text)
        assert l1 == l0 + 1 and i1 == i0 + n_items, (p, seen)
        if runs is not None:
            assert ("%d run%s," % (runs, "" if runs == 1 else "s")) in text, text


SCRIPTS = {  # tools/tpp_replay --script pack_a / pack_b / unpack_c (fp32-pack-gemm-operand-*.mlir, fp32-unpack-*.mlir)
    "pack_a": lambda: (pack(512, 1024), [512 * 1024]),
    "pack_b": lambda: (pack(1024, 512, perm=True), [1024 * 512]),
    "unpack_c": lambda: (unpack(512, 512), [512 * 512]),
}


@pytest.mark.parametrize("mode", [1, 2], ids=["direct", "scheduler"])
@pytest.mark.parametrize("script", sorted(SCRIPTS))
def test_pack_scripts_replay_as_one_relayout_grid(rtq, script, mode):
    rtq.set_tile_queue(mode)
    rng = np.random.default_rng(1)
    (items, nout, (m, n, ldi, ldo)), sizes = SCRIPTS[script]()
    srcs = sources(rng, F32, sizes)
    got, seen = run(rtq, IDENTITY, F32, (m, n, ldi, ldo), 0, items, srcs, nout)
    assert_grid_from_second_pass(seen, len(items), runs=1)
    assert "of them 16-byte" in seen[-1][1] and " 1 of them" in seen[-1][1], seen[-1][1]
    assert np.array_equal(got, reference(IDENTITY, F32, (m, n, ldi, ldo), items, srcs, nout))


CASES = {  # (kind, dtype, pattern)
    "identity_f32_pack": (IDENTITY, F32, lambda: pack(256, 512)),
    "identity_f32_unpack": (IDENTITY, F32, lambda: unpack(256, 512)),
    "identity_bf16_pack_perm": (IDENTITY, BF16, lambda: pack(512, 256, perm=True)),
    "identity_bf16_unpack": (IDENTITY, BF16, lambda: unpack(256, 512)),
    "vnni2_bf16_weight": (VNNI2, BF16, lambda: pack(512, 256, perm=True)),  # [K][N] -> [NB][KB][16][32][2]
    "identity_f32_64x48": (IDENTITY, F32, lambda: pack(256, 192, bm=64, bn=48)),
    "vnni2_bf16_64x64": (VNNI2, BF16, lambda: pack(256, 256, bm=64, bn=64)),
}


def exact_case(rt, name, threads=1):
    kind, dt, pat = CASES[name]
    items, nout, shape = pat()
    rng = np.random.default_rng(7)
    R = shape[2]
    srcs = sources(rng, dt, [max(oi for _, oi, _ in items) + (shape[0] - 1) * R + shape[1]])
    ref = reference(kind, dt, shape, items, srcs, nout)
    got, seen = run(rt, kind, dt, shape, 0, items, srcs, nout, threads=threads)
    return got, ref, seen, len(items), kind, dt, shape, items, srcs, nout


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_exact_under_poison_on_off_and_unqueued(rtq, name):
    got, ref, seen, n_items, kind, dt, shape, items, srcs, nout = exact_case(rtq, name)
    assert_grid_from_second_pass(seen, n_items, runs=1)
    assert np.array_equal(got, ref), name  # the guard bands and every byte between the blocks: still the poison
    rtq.set_relayout_grid(False)
    off, seen_off = run(rtq, kind, dt, shape, 0, items, srcs, nout)
    assert seen_off[-1][0] == seen[-1][0] and not seen_off[-1][1].startswith("relayout grid")
    rtq.set_relayout_grid(True)
    rtq.set_tile_queue(0)
    alone, _ = run(rtq, kind, dt, shape, 0, items, srcs, nout, passes=1)
    assert np.array_equal(off, ref) and np.array_equal(alone, ref), name


def test_interleaved_callers_give_the_same_runs(rtq):
    got, ref, seen, n_items, *_ = exact_case(rtq, "vnni2_bf16_weight", threads=4)
    assert_grid_from_second_pass(seen, n_items, runs=1)
    assert np.array_equal(got, ref)


def test_two_tensors_through_one_handle_are_two_runs_of_one_launch(rtq):
    """pack A (256x1024) and pack W (1024x1024, [NB][KB] blocks) of one layer: the same handle [32,32,1024,32], one group"""
    a_items, a_out, shape = pack(256, 1024)
    w_items, w_out, _ = pack(1024, 1024, perm=True)
    items = a_items + [(1, oi, a_out + 512 + oo) for _, oi, oo in w_items]  # W's blocks behind A's (512 elements apart)
    items = [items[i] for i in np.random.default_rng(3).permutation(len(items))]  # program order does not matter
    nout = a_out + 512 + w_out
    rng = np.random.default_rng(5)
    srcs = sources(rng, F32, [256 * 1024, 1024 * 1024])
    got, seen = run(rtq, IDENTITY, F32, shape, 0, items, srcs, nout)
    assert_grid_from_second_pass(seen, len(items), runs=2)
    assert np.array_equal(got, reference(IDENTITY, F32, shape, items, srcs, nout))


def _non_grid(kind_of_break):
    items, nout, shape = pack(256, 256)
    flags = 0
    if kind_of_break == "hole":
        items = items[:37] + items[38:]
    elif kind_of_break == "duplicate":
        items[21] = (0, items[20][1], items[21][2])  # block 20's source copied twice, block 21's never
    elif kind_of_break == "displaced":
        items[45] = (0, items[45][1], nout)  # one output off the grid (behind the others)
        nout += T * T
    elif kind_of_break == "broadcast":
        flags = 4  # column broadcast (XsmmEnum.td: BCAST_COL)
    elif kind_of_break == "ldo":
        items, nout, shape = pack(256, 256, ldo=40)  # strided outputs: 8 columns of every block row are not written
    return items, nout, shape, flags


@pytest.mark.parametrize("brk", ["hole", "duplicate", "displaced", "broadcast", "ldo"])
def test_non_grids_stay_on_the_item_kernel(rtq, brk):
    from oracle import pyoracle as orc
    items, nout, shape, flags = _non_grid(brk)
    m, n, ldi, ldo = shape
    rng = np.random.default_rng(11)
    src = np.full(256 * 256 + 2 * GUARD, -7.0, np.float32)
    src[GUARD:GUARD + 256 * 256] = rng.uniform(-1, 1, 256 * 256).astype(np.float32)
    ref = np.full(nout + 2 * GUARD, 0x7fc0dead, np.uint32).view(np.float32)
    for _, oi, oo in items:
        orc.unary(IDENTITY, F32, m, n, ldi, ldo, flags, src, GUARD + oi, ref, GUARD + oo)
    before = rtq.relayout_grid_stats()
    got, seen = run(rtq, IDENTITY, F32, shape, flags, items, [src.view(np.uint32)], nout)
    assert seen[-1][0] == before, (brk, seen)
    assert np.array_equal(got, ref.view(np.uint32)), brk


def test_unaligned_bases_take_the_element_path(rtq):
    items, nout, shape = pack(256, 256)
    rng = np.random.default_rng(13)
    srcs = sources(rng, F32, [256 * 256], base_shift=1)
    got, seen = run(rtq, IDENTITY, F32, shape, 0, items, srcs, nout, base_shift=1)
    if seen[-1][1].startswith("relayout grid"):
        assert " 0 of them 16-byte" in seen[-1][1], seen[-1][1]
    assert np.array_equal(got, reference(IDENTITY, F32, shape, items, srcs, nout, base_shift=1))


@pytest.mark.parametrize("name", ["identity_bf16_pack_perm", "vnni2_bf16_weight", "identity_f32_64x48"])
def test_element_path_on_shifted_bases(rtq, name):
    """bases one element off 16 bytes: the grid takes the kernel's element path (bf16 identity, the scalar VNNI-2 branch, f32)"""
    kind, dt, pat = CASES[name]
    items, nout, shape = pat()
    rng = np.random.default_rng(17)
    srcs = sources(rng, dt, [max(oi for _, oi, _ in items) + (shape[0] - 1) * shape[2] + shape[1]], base_shift=1)
    got, seen = run(rtq, kind, dt, shape, 0, items, srcs, nout, base_shift=1)
    assert_grid_from_second_pass(seen, len(items), runs=1)
    assert " 0 of them 16-byte" in seen[-1][1], seen[-1][1]
    assert np.array_equal(got, reference(kind, dt, shape, items, srcs, nout, base_shift=1)), name


def test_item_launch_after_a_grid_clears_the_grid_text(rtq):
    """a relayout grid names itself in last_grouped_kernel; a later group launched from gathered items does not keep that text"""
    items, nout, shape = pack(256, 352)  # (a handle no other test records: no earlier segment of it in the trace cache)
    srcs = sources(np.random.default_rng(19), F32, [256 * 352])
    _, seen = run(rtq, IDENTITY, F32, shape, 0, items, srcs, nout)
    assert seen[-1][1].startswith("relayout grid")
    h = rtq.unary_dispatch(5, F32, T, T, T, T, 0)  # relu tiles: a new group, recorded (not a complete replay)
    x = to_dev(np.zeros(64 * T * T, np.float32).view(np.uint32))
    for b in range(64):
        rtq.unary(F32, h, x, b * T * T, x, b * T * T)
    rtq.synchronize()
    assert not rtq.last_grouped_kernel().startswith("relayout grid"), rtq.last_grouped_kernel()


def test_strict_mode_keeps_relayout_grids():
    env = {k: v for k, v in os.environ.items() if k not in ("TPP_HIP_STRICT", "TPP_HIP_TILE_QUEUE", "TPP_HIP_ASYNC", "TPP_HIP_RELAYOUT_GRID")}
    env["TPP_HIP_STRICT"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--strict-worker"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["strict"] == 1
    for name in CASES:
        assert d[name]["exact"] and d[name]["grid"], (name, d[name])


def _strict_worker():
    rt = pkg.get_runtime()
    rt.set_async(True)
    rt.set_tile_queue(1)
    out = {"strict": int(rt.get_strict())}
    for name in CASES:
        got, ref, seen, *_ = exact_case(rt, name)
        out[name] = {"exact": bool(np.array_equal(got, ref)), "grid": seen[-1][1].startswith("relayout grid")}
    rt.synchronize()
    print(json.dumps(out))


if __name__ == "__main__" and "--strict-worker" in sys.argv:
    _strict_worker()
