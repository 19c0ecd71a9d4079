// brgemm_bf16_lw_chain_widths.hip - a MIXED-WIDTH chain of bf16 layers in one launch (opt-in: xsmm_hip_set_chain_widths): the instances of
// brgemm_bf16_lw in launch mode BLW_CHAIN_WIDTHS and their launcher. The kernel, its loader and launch_blw_t are brgemm_bf16_lw.hip's, included
// here with its own launchers and instances compiled out (BLW_KERNEL_ONLY), the arrangement of brgemm_bf16_lw_chain_ragged.hip: the code
// object of brgemm_bf16_lw.hip is pinned to the 120 instances of the launch table (tests/test_blw_launch_table.py), this mode lies beside
// the table (brgemm_bf16_lw_launch.h: blw_chain_widths_instance_exists, blw_chain_widths_launch_ok). The schedule: brgemm_bf16_lw_chain_widths.h.
#define BLW_KERNEL_ONLY
#include "brgemm_bf16_lw.hip"

namespace tpp {

// instance I of the 4 tiles x 3 B images x 2 chunks per barrier, compiled where blw_chain_widths_instance_exists says so (18 of the 24)
template <int I> static bool blw_chain_widths_try(int tile, int sup, int b_kind, const ChainArgs &a, hipStream_t s, hipError_t &e) {
  constexpr int TILE = I / 6, FB = 2 * (I / 2 % 3), SUP = 1 + I % 2;
  if constexpr (blw_chain_widths_instance_exists(TILE, FB, SUP)) {
    if (tile == TILE && b_kind == FB && sup == SUP) {
      constexpr BlwTile t = BLW_TILES[TILE];
      e = launch_blw_t<t.wm, t.wn, t.wk, t.tm, t.tn, t.nslot, t.nla, t.nlb, SUP, true, FB, BLW_CHAIN_WIDTHS>(a, s);
      return true;
    }
  }
  return false;
}
template <int... I> static hipError_t blw_chain_widths_seq(std::integer_sequence<int, I...>, int tile, int sup, int b_kind, const ChainArgs &a, hipStream_t s) {
  hipError_t e = hipErrorInvalidValue;
  (void)(blw_chain_widths_try<I>(tile, sup, b_kind, a, s, e) || ...);
  return e;
}

// The caller guarantees what launch_bf16_chain's caller does - co-residency (m / BM * max_l(n(l) / BN) workgroups at most the stream's
// compute units), beta = 0, disjoint buffers, ONE kind of B operand - and counters for m / BM row blocks that have received
// (a.target - 1) * (n(l) / BN) arrivals each: a.target is the epoch, a.L[l].pad = n(l), a.n = the widest layer's n.
// blw_chain_widths_launch_ok is what this refuses (hipErrorInvalidValue, nothing launched). Two chunks per barrier as launch_bf16_chain
// picks them: on the tiles that have such instances when EVERY layer has an even chunk count (a workgroup's active layers then start at
// even ring slots whichever it skips).
hipError_t launch_bf16_chain_widths(int tile, int b_kind, const ChainArgs &a, hipStream_t s) {
  BlwWidthsShape h{a.m, a.nlayers, {}, {}, {}};
  const int nl = a.nlayers < 1 ? 1 : a.nlayers > CH_MAXL ? CH_MAXL : a.nlayers;
  int widest = 0;
  for (int l = 0; l < nl; ++l) {
    h.n[l] = a.L[l].pad, h.k[l] = a.L[l].k, h.br[l] = a.L[l].br;
    if (h.n[l] > widest) widest = h.n[l];
  }
  if (!blw_chain_widths_launch_ok(tile, b_kind, h) || a.n != widest) return hipErrorInvalidValue;
  int sup = blw_tile_sup2(tile) ? 2 : 1;
  for (int l = 0; l < nl; ++l)
    if ((a.L[l].br * (a.L[l].k / BLW_BK)) & 1) sup = 1;
  return blw_chain_widths_seq(std::make_integer_sequence<int, 24>{}, tile, sup, b_kind, a, s);
}

} // namespace tpp
