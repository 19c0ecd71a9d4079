// brgemm_bf16_dma256_images.h - the three B images of the 256x256 bf16 tile (brgemm_bf16_dma256.hip), written once as plain functions: which
// bytes of global memory each LDS-DMA instruction of a chunk brings to which bytes of the B slot, where each fragment read of the MFMA waves
// looks, and which (k, column) values it hands its lane. The kernel, its launcher and a CPU test (tests/test_dma256_images.py) all include
// this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// A chunk is 32 k-values of the tile's 256 columns: 16 KiB of B in every image, brought by 16 instructions of 1 KiB (instruction v = 4 *
// wave + u, u = 0 .. 3; an LDS-DMA instruction writes lane i's 16 bytes at byte 16 i of its span, so every swizzle is on the SOURCE side).
//   image 0, VNNI-2 [k/2][ldb][2]: 16 pair-rows of 256 dwords as they are; instruction v = pair-row v. A lane's eight k of a k-step are four
//            dwords one pair-row apart: two ds_read2st64_b32.
//   image 2, flat [k][ldb]: 32 rows of 512 bytes; instruction v = rows 2v and 2v + 1; the eight 64-byte blocks of a row are XORed with row & 3
//            (the 128-wide loader-wave image's rule: the four rows a 16-lane group of a transpose read names land in the four quarters of a
//            bank row). A lane's eight k are two ds_read_b64_tr_b16 four rows apart.
//   image 4, VNNI-4 [k/4][ldb][4]: 8 k-group rows of 2 KiB ([256 columns][4 k]) as they are; instruction v = half v & 1 of k-group row v / 2.
//            A lane's eight k are two 8-byte reads one k-group row apart.
// In every image the reads of k-step ks + 1 lie D256_KS_STEP bytes behind those of k-step ks and the second read of a fragment D256_H_STEP
// bytes behind the first, so the kernel's issue schedule is one for all three.
#pragma once

namespace tpp {

constexpr int D256_BM = 256, D256_BN = 256, D256_BK = 32;  // the workgroup tile and the k of a chunk
constexpr int D256_A_SLOT = D256_BM * D256_BK * 2;          // A image of a chunk: [256 rows][64 B]
constexpr int D256_B_SLOT = D256_BK * D256_BN * 2;          // B image of a chunk: 16 KiB in every image
constexpr int D256_B_INSTR = 16;                            // LDS-DMA instructions per chunk of B, 1 KiB each
constexpr int D256_KS_STEP = 8192, D256_H_STEP = 2048;      // fragment reads: from k-step 0 to 1, from a fragment's first read to its second

constexpr bool d256_image_ok(int img) { return img == 0 || img == 2 || img == 4; }
// k-values per global row of the image (a pair-row, a flat row, a k-group row) and the row's stride in bytes
constexpr int d256_b_row_k(int img) { return img == 0 ? 2 : img == 2 ? 1 : 4; }
constexpr long long d256_b_row_bytes(int img, long long ldb) { return 2 * d256_b_row_k(img) * ldb; }
// elements from the start of a global row to column n0, and from a chunk to the next one of the same batch element
constexpr long long d256_b_col_elems(int img, long long n0) { return d256_b_row_k(img) * n0; }
constexpr long long d256_b_chunk_elems(long long ldb) { return (long long)D256_BK * ldb; }

// ---- the writer: LDS-DMA instruction v (0 .. 15) of a chunk, lane i (0 .. 63) -------------------------------------------------------------
// global row of the chunk the lane's 16 bytes come from (0 .. 32 / d256_b_row_k - 1) ...
constexpr int d256_b_dma_row(int img, int v, int lane) { return img == 0 ? v : img == 2 ? 2 * v + (lane >> 5) : v >> 1; }
// ... and their byte offset inside the tile's 256 columns of that row (swz = false: the flat image without its swizzle, for the CPU test only)
constexpr int d256_b_dma_src(int img, int v, int lane, bool swz = true) {
  return img == 0 ? 16 * lane : img == 2 ? (((lane & 31) ^ (swz ? (d256_b_dma_row(2, v, lane) & 3) << 2 : 0)) << 4) : 1024 * (v & 1) + 16 * lane;
}
// the lane's source offset from (first row of the chunk, column n0), in bytes: what the instruction carries as its VGPR offset
constexpr unsigned d256_b_dma_voff(int img, int v, int lane, long long ldb) {
  return (unsigned)(d256_b_dma_row(img, v, lane) * d256_b_row_bytes(img, ldb) + d256_b_dma_src(img, v, lane));
}
// where they land in the B slot
constexpr int d256_b_dma_lds(int v, int lane) { return 1024 * v + 16 * lane; }
// what the launcher asks of ldb: 16-byte pieces at every lane's source, and the largest lane offset in 31 bits
constexpr bool d256_b_ldb_ok(int img, long long ldb) {
  return ldb >= D256_BN && ldb % (img == 0 ? 4 : img == 2 ? 8 : 2) == 0 && (D256_BK / d256_b_row_k(img)) * d256_b_row_bytes(img, ldb) < (1ll << 31);
}

// ---- the reader: wave column wn (0 / 1), column tile j (0 .. 3), k-step ks (0 / 1), lane, read h (0 / 1) of the fragment ---------------------
// byte address inside the B slot. Image 0: read h is a ds_read2st64_b32 of this dword and the one 1024 bytes behind it; image 2: the
// address the lane NAMES to ds_read_b64_tr_b16 - lane 4q + p of a 16-lane group names row q, columns 4p .. 4p + 3 of the group's [4 k][16
// columns] block; image 4: an 8-byte read.
constexpr int d256_b_frag_lds(int img, int wn, int j, int ks, int lane, int h, bool swz = true) {
  return D256_KS_STEP * ks + D256_H_STEP * h +
         (img == 0   ? ((4 * (lane >> 5)) * D256_BN + 128 * wn + 32 * j + (lane & 31)) * 4
          : img == 2 ? (8 * (lane >> 5) + ((lane & 15) >> 2)) * 512 + (((4 * wn + j) ^ (swz ? (lane & 15) >> 2 : 0)) << 6) + ((lane >> 4) & 1) * 32 + (lane & 3) * 8
                     : (2 * (lane >> 5)) * 2048 + (128 * wn + 32 * j + (lane & 31)) * 8);
}
// what the read hands the lane: k-values d256_b_frag_k .. + 3 of the chunk, of column d256_b_frag_col of the tile - its MFMA operand
// registers 2h and 2h + 1 (two bf16 each, ascending k)
constexpr int d256_b_frag_k(int ks, int lane, int h) { return 16 * ks + 8 * (lane >> 5) + 4 * h; }
constexpr int d256_b_frag_col(int wn, int j, int lane) { return 128 * wn + 32 * j + (lane & 31); }
// the lane map of ds_read_b64_tr_b16 (tools/ubench/tr16_probe.hip pins it): element q (0 .. 3) of lane i's result is the 16-bit element
// d256_tr16_elem(i) of the 8 bytes that lane d256_tr16_lane(i, q) of the same 16-lane group names
constexpr int d256_tr16_lane(int lane, int q) { return (lane & ~15) + 4 * q + ((lane & 15) >> 2); }
constexpr int d256_tr16_elem(int lane) { return lane & 3; }

} // namespace tpp
