// brgemm_bf16_dma256_edge.h - the edge tiles of the 256x256 bf16 tile (brgemm_bf16_dma256_edge.hip, xsmm_hip_set_dma256_edge), written once as
// plain functions: where workgroup (tm, tn) of the ceil-divided grid puts its tile, and which of the tile's 256 x 256 elements it stores.
// The kernel, its launcher and a CPU test (tests/test_dma256_edge_map.py) all include this file. Nothing here needs a device: it compiles
// with any C++14 host compiler.
//
// The grid is ceil(m / 256) x ceil(n / 256) workgroups. Every tile but the last of a dimension starts at 256 t; the last one is shifted
// back to end with the matrix (m - 256, n - 256), computes all its 256 x 256 elements from operands that lie inside the matrix and stores
// only the rows from 256 tm and the columns from 256 tn on - what lies in front of them is the neighbour's. n % 8 == 0 makes the column
// shift a whole number of 16-byte pieces of C, of all three B images and of the bias row.
#pragma once

namespace tpp {

constexpr int D256E_T = 256; // the tile's rows and columns

// what the launcher asks of an extent (m or n), and the tiles it then takes
constexpr bool d256e_extent_ok(long long x) { return x >= D256E_T; }
constexpr int d256e_tiles(int x) { return (x + D256E_T - 1) / D256E_T; }
// first row (column) of tile t of an extent of x rows (columns)
constexpr int d256e_origin(int t, int x) { return t * D256E_T < x - D256E_T ? t * D256E_T : x - D256E_T; }
// rows (columns) at the front of tile t that the tile in front of it owns: 0 for every tile that is not shifted
constexpr int d256e_skip(int t, int x) { return t * D256E_T - d256e_origin(t, x); }
// does workgroup (tm, tn) of an m x n output store element (r, c)?
constexpr bool d256e_owns(int tm, int tn, int m, int n, int r, int c) {
  return r >= tm * D256E_T && r < d256e_origin(tm, m) + D256E_T && c >= tn * D256E_T && c < d256e_origin(tn, n) + D256E_T;
}

} // namespace tpp
