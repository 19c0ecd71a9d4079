// driver.cpp - TEST INFRASTRUCTURE for tests/test_blw_launch_table.py, never part of the product library.
//
// Prints the launch table of tpp-mlir_amd/csrc/brgemm_bf16_lw_launch.h, compiled as plain host C++:
//   inst <mode> <multi> <tile> <b_kind> <sup> : <WM WN WK TM TN NSLOT NLA NLB> : <BM> <BN> : <the kernel's symbol>
// for every combination blw_instance_exists holds for, then answers blw_launch_ok for the launches on its standard input, one per line:
//   <mode> <tile> <b_kind> <chain> <m> <n> <nlayers> <groups> <k of layer 0> <br of layer 0> [<k> <br> of further layers]   ->  ok 0 / ok 1
// (layers the line does not give repeat the last one given).
#include "brgemm_bf16_lw_launch.h"
#include <cstdio>

using namespace tpp;

// the whole table is usable in constant expressions: the plain 64x64 layer exists, a ragged k has no two-chunk instance
static_assert(blw_instance_exists(BLW_LAYER, false, 1, 0, 2) && !blw_instance_exists(BLW_KEDGE, false, 1, 0, 2), "");
static_assert(BLW_TILES[0].bm() == 32 && BLW_TILES[3].bn() == 128 && BLW_TILES[4].bn() == 32, "");
static_assert(blw_launch_ok(BLW_LAYER, 0, 0, BlwShape{false, 32, 64, 1, 0, {64}, {1}}), "");

int main() {
  for (int mode = 0; mode < BLW_MODES; ++mode)
    for (int multi = 0; multi < 2; ++multi)
      for (int tile = -1; tile <= BLW_NTILES; ++tile)
        for (int b_kind = -1; b_kind <= 5; ++b_kind)
          for (int sup = 0; sup <= 4; ++sup) {
            if (!blw_instance_exists(mode, multi != 0, tile, b_kind, sup)) continue;
            const BlwTile &t = BLW_TILES[tile];
            const int v[8] = {t.wm, t.wn, t.wk, t.tm, t.tn, t.nslot, t.nla, t.nlb};
            printf("inst %d %d %d %d %d :", mode, multi, tile, b_kind, sup);
            for (int x : v) printf(" %d", x);
            printf(" : %d %d : _ZN3tpp14brgemm_bf16_lwI", t.bm(), t.bn());
            for (int x : v) printf("Li%dE", x);
            printf("Li%dELb%dELi%dELi%dEEEvNS_9ChainArgsE\n", sup, multi, b_kind, mode);
          }
  int mode, tile, b_kind, chain;
  BlwShape a{};
  while (scanf("%d %d %d %d %d %d %d %d", &mode, &tile, &b_kind, &chain, &a.m, &a.n, &a.nlayers, &a.groups) == 8) {
    a.chain = chain != 0;
    int given = 0, k, br;
    char c;
    while (given < BLW_MAXL && scanf("%d %d%c", &k, &br, &c) == 3) {
      a.k[given] = k, a.br[given] = br, ++given;
      if (c == '\n') break;
    }
    for (int l = given; l < BLW_MAXL; ++l) a.k[l] = a.k[given - 1], a.br[l] = a.br[given - 1];
    printf("ok %d\n", blw_launch_ok(mode, tile, b_kind, a) ? 1 : 0);
  }
  return 0;
}
