// brgemm_bf16_lw_chain_ragged.hip - a RAGGED-WIDTH chain of bf16 layers in one launch (opt-in: xsmm_hip_set_chain_ragged): the instances of
// brgemm_bf16_lw in launch mode BLW_CHAIN_RAGGED and their launcher. The kernel, its loader and launch_blw_t are brgemm_bf16_lw.hip's, included
// here with its own launchers and instances compiled out (BLW_KERNEL_ONLY). A translation unit of its own: the code
// object of brgemm_bf16_lw.hip is pinned to the 120 instances of the launch table (tests/test_blw_launch_table.py), this mode lies beside
// the table (brgemm_bf16_lw_launch.h: blw_chain_ragged_instance_exists, blw_chain_ragged_launch_ok). The schedule: brgemm_bf16_lw_chain_ragged.h.
#define BLW_KERNEL_ONLY
#include "brgemm_bf16_lw.hip"

namespace tpp {

// instance I of the 4 tiles x 3 B images, compiled where blw_chain_ragged_instance_exists says so
template <int I> static bool blw_chain_ragged_try(int tile, int b_kind, const ChainArgs &a, hipStream_t s, hipError_t &e) {
  constexpr int TILE = I / 3, FB = 2 * (I % 3);
  if constexpr (blw_chain_ragged_instance_exists(TILE, FB)) {
    if (tile == TILE && b_kind == FB) {
      constexpr BlwTile t = BLW_TILES[TILE];
      e = launch_blw_t<t.wm, t.wn, t.wk, t.tm, t.tn, t.nslot, t.nla, t.nlb, 1, true, FB, BLW_CHAIN_RAGGED>(a, s);
      return true;
    }
  }
  return false;
}
template <int... I> static hipError_t blw_chain_ragged_seq(std::integer_sequence<int, I...>, int tile, int b_kind, const ChainArgs &a, hipStream_t s) {
  hipError_t e = hipErrorInvalidValue;
  (void)(blw_chain_ragged_try<I>(tile, b_kind, a, s, e) || ...);
  return e;
}

// The caller guarantees what launch_bf16_chain's caller does - co-residency (ceil(m / BM) * ceil(n / BN) workgroups at most the stream's
// compute units), beta = 0, disjoint buffers, ONE kind of B operand - and counters for ceil(m / BM) row blocks, a.target a multiple of
// ceil(n / BN) arrivals. blw_chain_ragged_launch_ok is what this refuses (hipErrorInvalidValue, nothing launched).
hipError_t launch_bf16_chain_ragged(int tile, int b_kind, const ChainArgs &a, hipStream_t s) {
  BlwShape h{true, a.m, a.n, a.nlayers, 0, {}, {}};
  for (int l = 0; l < (a.nlayers < 1 ? 1 : a.nlayers > CH_MAXL ? CH_MAXL : a.nlayers); ++l) h.k[l] = a.L[l].k, h.br[l] = a.L[l].br;
  if (!blw_chain_ragged_launch_ok(tile, b_kind, h)) return hipErrorInvalidValue;
  return blw_chain_ragged_seq(std::make_integer_sequence<int, 12>{}, tile, b_kind, a, s);
}

} // namespace tpp
