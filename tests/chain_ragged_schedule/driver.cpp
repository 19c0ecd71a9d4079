// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_ragged_schedule.py, never part of the product library.
//
// Walks tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_ragged.h - the header the ragged-width chain kernel includes - as plain host C++. For every ring
// depth NSLOT in {4, 6, 8} and a list of chains (every pair of layers over k in {64 .. 1000} x br in {1, 2, 3}, and seeded samples of three
// and four layers):
//   chain <nslot> <L> <k>:<br> ...
//   <layer> <chunk> <batch element> <first k> <skipped halves> <parts of k-steps 0 .. 3> <slot> <loader's slot> <loader's first k> <MFMA loop's slot> <MFMA loop's skip>
// one line per chunk in the order both sides walk them. <slot>, <first k>, <skipped halves> and <parts> are the header's functions of
// (layer, chunk); the loader's columns come from a walk the way blw_loader makes it (slot = s0 at a layer's first request, then the next
// slot; the first k advanced by 64, by bkedge_step into the last chunk, and back to 0 behind it), the MFMA loop's from a walk the way the
// kernel's K loop makes it (slot = s0, then the next slot; kc counted up to chain_ragged_test_period, the layer's skip on that chunk).
#include "brgemm_bf16_lw_chain_ragged.h"
#include <initializer_list>
#include <stdio.h>
#include <vector>

using namespace tpp;

static_assert(chain_ragged_layer_skip(1024) == 0 && chain_ragged_layer_skip(1000) == 3 && chain_ragged_layer_skip(72) == 7 && chain_ragged_layer_skip(784) == 6, "");
static_assert(chain_ragged_chunks(64) == 1 && chain_ragged_chunks(200) == 4 && chain_ragged_chunk_k0(200, 3) == 136 && chain_ragged_chunk_k0(200, 7) == 136, "");
static_assert(chain_ragged_step_part(1024, 15, 0) == BKEDGE8_WHOLE && chain_ragged_step_part(72, 1, 3) == BKEDGE8_UPPER && chain_ragged_step_part(72, 1, 2) == BKEDGE8_NONE, "");
static_assert(chain_ragged_k_ok(64) && chain_ragged_k_ok(72) && !chain_ragged_k_ok(56) && !chain_ragged_k_ok(76), "");
static_assert(chain_ragged_col0(1, 72, 64) == 8 && chain_ragged_own_col(1, 72, 64) == 56 && chain_ragged_own_col(0, 72, 64) == 0 && chain_ragged_tiles_n(1000, 64) == 16, "");

static const int KS[12] = {64, 72, 80, 88, 96, 104, 112, 120, 128, 200, 784, 1000};

static void walk(int nslot, const std::vector<int> &k, const std::vector<int> &br) {
  const int L = (int)k.size();
  printf("chain %d %d", nslot, L);
  for (int l = 0; l < L; ++l) printf(" %d:%d", k[l], br[l]);
  printf("\n");
  int s0_loader = 0, s0_mfma = 0;
  for (int l = 0; l < L; ++l) {
    const int T = chain_ragged_layer_chunks(k[l], br[l]), kchunks = chain_ragged_chunks(k[l]), period = chain_ragged_test_period(k[l], T);
    const int s0 = chain_ragged_s0(l, k.data(), br.data(), nslot);
    int slot_l = s0_loader, k0_l = 0, kc_l = 0; // the loader's issue state
    int slot_m = s0_mfma, kc_m = 0;             // the MFMA loop's
    for (int c = 0; c < T; ++c) {
      const bool last = kc_m + 1 == period; // (the K loop's count: to the next chunk it tests)
      const int skip_m = last ? chain_ragged_layer_skip(k[l]) : 0;
      printf("%d %d %d %d %d %d%d%d%d %d %d %d %d %d\n", l, c, chain_ragged_batch(k[l], c), chain_ragged_chunk_k0(k[l], c), chain_ragged_skip_halves(k[l], c),
             chain_ragged_step_part(k[l], c, 0), chain_ragged_step_part(k[l], c, 1), chain_ragged_step_part(k[l], c, 2), chain_ragged_step_part(k[l], c, 3),
             chain_ragged_slot(s0, c, nslot), slot_l, k0_l, slot_m, skip_m);
      // the loader's advance (BLW_ISSUE, KEDGE): + 64, + k % 64 into the last chunk, the batch wrap behind it
      ++kc_l;
      if (kc_l == kchunks) k0_l = 0, kc_l = 0;
      else k0_l += kc_l + 1 == kchunks ? bkedge_step(k[l], kchunks - 2) : BKEDGE_BK;
      slot_l = chain_ragged_next_slot(slot_l, nslot);
      kc_m = last ? 0 : kc_m + 1;
      slot_m = chain_ragged_next_slot(slot_m, nslot);
    }
    s0_loader = chain_ragged_next_s0(s0_loader, k[l], br[l], nslot);
    s0_mfma = chain_ragged_next_s0(s0_mfma, k[l], br[l], nslot);
  }
}

int main() {
  unsigned seed = 12345u;
  auto rnd = [&](int n) { seed = seed * 1664525u + 1013904223u; return (int)((seed >> 8) % (unsigned)n); };
  for (int nslot : {4, 6, 8}) {
    for (int a = 0; a < 36; ++a)
      for (int b = 0; b < 36; ++b) walk(nslot, {KS[a / 3], KS[b / 3]}, {1 + a % 3, 1 + b % 3});
    for (int L : {3, 4})
      for (int i = 0; i < 200; ++i) {
        std::vector<int> k, br;
        for (int l = 0; l < L; ++l) k.push_back(KS[rnd(12)]), br.push_back(1 + rnd(3));
        walk(nslot, k, br);
      }
  }
  return 0;
}
