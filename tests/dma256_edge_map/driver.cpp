// Walks the edge-tile maps of the 256x256 bf16 tile (tpp-mlir_amd/csrc/brgemm_bf16_dma256_edge.h) on a CPU: for an m x n output every
// workgroup of the ceil-divided grid marks the elements d256e_owns gives it - and, as the control, all 256 x 256 elements of its tile.
// Prints facts; tests/test_dma256_edge_map.py asserts them.
//   driver <m> <n>
#include "brgemm_bf16_dma256_edge.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace tpp;

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const int m = atoi(argv[1]), n = atoi(argv[2]);
  if (!d256e_extent_ok(m) || !d256e_extent_ok(n)) return 3;
  const int tiles_m = d256e_tiles(m), tiles_n = d256e_tiles(n);
  std::vector<int> owned((size_t)m * n, 0), computed((size_t)m * n, 0);
  long outside = 0, origin_col_off8 = 0, skip_mismatch = 0, owned_outside_tile = 0;
  for (int tm = 0; tm < tiles_m; ++tm)
    for (int tn = 0; tn < tiles_n; ++tn) {
      const int m0 = d256e_origin(tm, m), n0 = d256e_origin(tn, n);
      if (m0 < 0 || n0 < 0 || m0 + D256E_T > m || n0 + D256E_T > n) ++outside;
      if (n0 % 8) ++origin_col_off8;
      // far from the tile (a lattice over the whole output, the last rows and columns included): nothing is owned there
      for (int r = 0; r < m; r = r + 61 < m || r == m - 1 ? r + 61 : m - 1)
        for (int c = 0; c < n; c = c + 67 < n || c == n - 1 ? c + 67 : n - 1)
          if (d256e_owns(tm, tn, m, n, r, c) && !(r >= m0 && r < m0 + D256E_T && c >= n0 && c < n0 + D256E_T)) ++owned_outside_tile;
      // the tile and a tile's width around it: every element
      for (int r = m0 - D256E_T < 0 ? 0 : m0 - D256E_T; r < m && r < m0 + 2 * D256E_T; ++r)
        for (int c = n0 - D256E_T < 0 ? 0 : n0 - D256E_T; c < n && c < n0 + 2 * D256E_T; ++c) {
          const bool in_tile = r >= m0 && r < m0 + D256E_T && c >= n0 && c < n0 + D256E_T;
          const bool own = d256e_owns(tm, tn, m, n, r, c);
          if (in_tile) ++computed[(size_t)r * n + c];
          if (own) ++owned[(size_t)r * n + c];
          if (own && !in_tile) ++owned_outside_tile;
          // the form the kernel's epilogue uses: local row / column at or behind the skip
          if (in_tile && own != (r - m0 >= d256e_skip(tm, m) && c - n0 >= d256e_skip(tn, n))) ++skip_mismatch;
        }
    }
  long once = 0, never = 0, more = 0, twice_unpredicated = 0, never_computed = 0;
  for (size_t i = 0; i < owned.size(); ++i) {
    once += owned[i] == 1, never += owned[i] == 0, more += owned[i] > 1;
    twice_unpredicated += computed[i] > 1, never_computed += computed[i] == 0;
  }
  printf("tiles %d %d\n", tiles_m, tiles_n);
  printf("origins outside %ld col_off8 %ld\n", outside, origin_col_off8);
  printf("owned once %ld never %ld more %ld outside_tile %ld skip_mismatch %ld\n", once, never, more, owned_outside_tile, skip_mismatch);
  printf("unpredicated twice %ld never %ld\n", twice_unpredicated, never_computed);
  return 0;
}
