// rt_relayout.h - RELAYOUT GRIDS: a recorded group of per-block identity / VNNI-2 unary invokes (a tensor.pack / unpack as the
// compiler lowers it) -> ONE launch of relayout.hip over a table of affine runs.
// Plain C++ over addresses (no queue state): runtime.cpp's tile queue calls relayout_decompose (detect_relayout, rt_rewrites.h), and
// tests/test_relayout_decompose.py compiles it on its own.
//
// LowerPacksAndUnpacks.cpp:45-49,112-121 turns a tensor.pack / unpack into one xsmm.unary identity per 32x32 (or m x n) block, and
// the bf16 weight's VNNI pack into one VNNI-2 invoke per block: hundreds of invokes of ONE handle whose pointers are affine in the
// block index. Through the tile queue they are one group, and as items they ran on unary_grouped_kernel (one workgroup per item, an
// element per lane per step: ~1 TB/s of read + write). When a recorded group qualifies -
//   * one unary handle, identity (f32 / bf16) or VNNI-2 (bf16, m even), no broadcast flags, m, n <= 64;
//   * its items split into at most RELAYOUT_MAX_RUNS runs, each an affine 2-D grid - block (r, c) reads in0 + r in_r + c in_c and
//     writes out0 + r out_r + c out_c, every (r, c) of R x C exactly once;
//   * every run writes ONE dense range (its blocks tile [out0, out0 + R C m n elements) with no gap: no strided outputs, ldo = n for
//     a pack, whole rows for an unpack), and the runs' input extents (first block's start to last block's end) are pairwise
//     disjoint. That is the whole rule. It refuses most broken grids - a hole, a duplicated or displaced block inside a tensor
//     leaves runs over one source whose extents overlap - but not all: a tensor missing its LAST block is two runs (7 x 8 + 1 x 7)
//     with disjoint extents and is accepted. Either way the runs cover exactly the recorded items, so the result is the items'. -
// a complete replay is ONE launch of relayout_grid_kernel; otherwise the group stays on unary_grouped_kernel unchanged.
// Items of a group have no dependence between them (the queue ends a group on one), so runs are formed by ADDRESS, not program order:
// the items are taken in output-address order (Segment::build sorts them so), a run's column count is the longest stretch of equal
// address steps, its rows follow while each repeats the first row shifted by one step. Items recorded from several calling threads
// in any interleaving, and two tensors packed through one handle (pack A and pack W of a layer), give the same runs.
// The result is a copy of raw words: bit for bit what the items would have written, whichever kernel writes it. So the path stays on
// in STRICT mode. TPP_HIP_RELAYOUT_GRID=0 / xsmm_hip_set_relayout_grid(0) switches it off (A/B runs).
#pragma once
#include "xsmm_desc.h"
#include <stdint.h>
#include <algorithm>
#include <cstdlib>
#include <vector>

namespace tpp {

constexpr int RELAYOUT_MAX_RUNS = 16;

struct RelayoutItem {
  uintptr_t in, out;
};

// items (any order) of one descriptor: op 1 identity / 28 VNNI-2, elements of `esz` bytes, m x n blocks, ldi / ldo. Fills runs[]
// (R, C, bases, strides, vec; wg0 is left to the caller) and returns their number, or -1 if the items are not such a set of runs.
inline int relayout_decompose(int64_t op, int esz, int64_t m, int64_t n, int64_t ldi, int64_t ldo, std::vector<RelayoutItem> items,
                              RelayoutRun *runs, int max_runs) {
  const size_t N = items.size();
  if (N < 2 || m <= 0 || n <= 0 || (esz != 2 && esz != 4)) return -1;
  const bool vnni = op == 28;
  if (vnni && (m & 1)) return -1;
  const int64_t blk = m * n;                                                           // elements one block writes
  const int64_t out_fp = vnni ? (m / 2 - 1) * 2 * ldo + 2 * n : (m - 1) * ldo + n;    // ... and the extent they span
  const int64_t in_fp = (m - 1) * ldi + n;
  std::sort(items.begin(), items.end(), [](const RelayoutItem &a, const RelayoutItem &b) { return a.out < b.out; });
  for (size_t i = 0; i < N; ++i)
    if (items[i].in % esz || items[i].out % esz || (i && items[i].out == items[i - 1].out)) return -1;
  auto din = [&](size_t a, size_t b) { return ((int64_t)items[b].in - (int64_t)items[a].in) / esz; };
  auto dout = [&](size_t a, size_t b) { return ((int64_t)items[b].out - (int64_t)items[a].out) / esz; };
  int nr = 0;
  std::vector<std::pair<int64_t, int64_t>> in_span; // [begin, end) in bytes, per run
  size_t p = 0;
  while (p < N) {
    if (nr == max_runs) return -1;
    int64_t ic = 0, oc = 0, ir = 0, orr = 0;
    size_t C = 1, R = 1;
    if (p + 1 < N) {
      ic = din(p, p + 1), oc = dout(p, p + 1);
      C = 2;
      while (p + C < N && din(p + C - 1, p + C) == ic && dout(p + C - 1, p + C) == oc) ++C;
      if (p + C < N) {
        ir = din(p, p + C), orr = dout(p, p + C);
        for (;;) {
          const size_t q = p + R * C;
          if (q + C > N) break;
          bool row = true;
          for (size_t c = 0; c < C && row; ++c)
            row = din(p, q + c) == (int64_t)R * ir + (int64_t)c * ic && dout(p, q + c) == (int64_t)R * orr + (int64_t)c * oc;
          if (!row) break;
          ++R;
        }
      }
    }
    const size_t cnt = R * C;
    // one dense output range (items never overlap: the group was proven conflict-free)
    if ((int64_t)(items[p + cnt - 1].out - items[p].out) / esz + out_fp != (int64_t)cnt * blk) return -1;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (size_t i = p; i < p + cnt; ++i) {
      lo = std::min(lo, (int64_t)items[i].in);
      hi = std::max(hi, (int64_t)items[i].in + in_fp * esz);
    }
    for (const auto &s : in_span)
      if (lo < s.second && s.first < hi) return -1;
    in_span.push_back({lo, hi});
    RelayoutRun &ru = runs[nr++];
    if (R > 1 && C > 1 && std::llabs(ic) > std::llabs(ir)) { // inner index = the smaller source step (consecutive workgroups on neighbouring source rows)
      ru.R = (int32_t)C, ru.C = (int32_t)R;
      ru.in_r = ic, ru.in_c = ir, ru.out_r = oc, ru.out_c = orr;
    } else {
      ru.R = (int32_t)R, ru.C = (int32_t)C;
      ru.in_r = ir, ru.in_c = ic, ru.out_r = orr, ru.out_c = oc;
    }
    ru.in = (const void *)items[p].in;
    ru.out = (void *)items[p].out;
    ru.wg0 = 0;
    // 16-byte pieces: identity moves 16 / esz elements per access, VNNI-2 reads 4 columns (8 bytes) of each row of a pair
    const int64_t v = vnni ? 4 : 16 / esz, vo = 16 / esz;
    ru.vec = items[p].in % (vnni ? 8 : 16) == 0 && items[p].out % 16 == 0 && n % v == 0 && ldi % v == 0 && (vnni ? ldo % 4 : ldo % vo) == 0 &&
             ru.in_r % v == 0 && ru.in_c % v == 0 && ru.out_r % vo == 0 && ru.out_c % vo == 0;
    p += cnt;
  }
  return nr;
}

} // namespace tpp
