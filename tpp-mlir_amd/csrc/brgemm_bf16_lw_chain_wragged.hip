// brgemm_bf16_lw_chain_wragged.hip - a RAGGED MIXED-WIDTH chain of bf16 layers in one launch (opt-in: xsmm_hip_set_chain_widths_ragged): the
// instances of brgemm_bf16_lw in launch mode BLW_CHAIN_WRAGGED and their launcher. The kernel, its loader and launch_blw_t are
// brgemm_bf16_lw.hip's, included here with its own launchers and instances compiled out (BLW_KERNEL_ONLY), the arrangement of
// brgemm_bf16_lw_chain_ragged.hip and brgemm_bf16_lw_chain_widths.hip: the code object of brgemm_bf16_lw.hip is pinned to the 120 instances of
// the launch table (tests/test_blw_launch_table.py), this mode lies beside the table (brgemm_bf16_lw_launch.h:
// blw_chain_wragged_instance_exists, blw_chain_wragged_launch_ok). The schedule: brgemm_bf16_lw_chain_wragged.h.
// Eleven instances, one chunk per barrier, none with scratch: tiles 0 .. 3 with the VNNI-2, flat and VNNI-4 images, less the 64x128 tile
// with the VNNI-2 image (it would need 72 bytes of scratch per lane, as it needs 76 in BLW_CHAIN_RAGGED).
#define BLW_KERNEL_ONLY
#include "brgemm_bf16_lw.hip"

namespace tpp {

// instance I of the 4 tiles x 3 B images, compiled where blw_chain_wragged_instance_exists says so
template <int I> static bool blw_chain_wragged_try(int tile, int b_kind, const ChainArgs &a, hipStream_t s, hipError_t &e) {
  constexpr int TILE = I / 3, FB = 2 * (I % 3);
  if constexpr (blw_chain_wragged_instance_exists(TILE, FB)) {
    if (tile == TILE && b_kind == FB) {
      constexpr BlwTile t = BLW_TILES[TILE];
      e = launch_blw_t<t.wm, t.wn, t.wk, t.tm, t.tn, t.nslot, t.nla, t.nlb, 1, true, FB, BLW_CHAIN_WRAGGED>(a, s);
      return true;
    }
  }
  return false;
}
template <int... I> static hipError_t blw_chain_wragged_seq(std::integer_sequence<int, I...>, int tile, int b_kind, const ChainArgs &a, hipStream_t s) {
  hipError_t e = hipErrorInvalidValue;
  (void)(blw_chain_wragged_try<I>(tile, b_kind, a, s, e) || ...);
  return e;
}

// The caller guarantees what launch_bf16_chain's caller does - co-residency (ceil(m / BM) * max_l ceil(n(l) / BN) workgroups at most the
// stream's compute units), beta = 0, disjoint buffers, ONE kind of B operand - and counters for ceil(m / BM) row blocks that have received
// (a.target - 1) * ceil(n(l) / BN) arrivals each: a.target is the epoch, a.L[l].pad = n(l), a.n = the widest layer's n.
// blw_chain_wragged_launch_ok is what this refuses (hipErrorInvalidValue, nothing launched).
hipError_t launch_bf16_chain_wragged(int tile, int b_kind, const ChainArgs &a, hipStream_t s) {
  BlwWidthsShape h{a.m, a.nlayers, {}, {}, {}};
  const int nl = a.nlayers < 1 ? 1 : a.nlayers > CH_MAXL ? CH_MAXL : a.nlayers;
  int widest = 0;
  for (int l = 0; l < nl; ++l) {
    h.n[l] = a.L[l].pad, h.k[l] = a.L[l].k, h.br[l] = a.L[l].br;
    if (h.n[l] > widest) widest = h.n[l];
  }
  if (!blw_chain_wragged_launch_ok(tile, b_kind, h) || a.n != widest) return hipErrorInvalidValue;
  return blw_chain_wragged_seq(std::make_integer_sequence<int, 12>{}, tile, b_kind, a, s);
}

} // namespace tpp
