// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_call_switches.py, never part of the product library.
//
// The single-call launch decision (tpp-mlir_amd/csrc/gemm_plan.h plan_gemm, plan_gemm_call) under every set of the eight mode switches
// xsmm_hip_set_dma256_edge, _edge_tiles, _edge_k, _edge_k_bf16, _edge_k8_bf16, _dma256_images, _tail_split and _f32_halves, with
// xsmm_hip_force_split as part of the context. Plain host C++ linked with the unchanged gemm_plan.cpp.
//   driver sweep <compute units> <strict 0 | 1>   checks a .. e of the test's docstring over the lattice; FAIL lines, REFUSED lines, counts, "OK"
//   driver sweep <compute units> <strict> quick   the same over an eighth of the shape lattice and the whole sub-lattice (the sanitizer build)
//   driver table                                  the golden table (tests/golden/gemm_call_switches.txt)
// A descriptor prints as
//   <form> <m>x<n>x<k> ld<lda>,<ldb>,<ldc> s<stride_a>,<stride_b> e<epilogue> f<forced>[ vc] : v<variant> <name>[ gf][ vf]
// a call as br<batch> a<A,B>/<C>/<D alignment in bytes>, a switch set as the + joined names of its members, and a launch as
//   <launcher> t<tile> s<split> b<B image>[ even][ vec][ g<generic>][ tail<tiles>x<workgroups>][ edge][ edge_k][ edge_k8][ halves] "<text>"
#include "gemm_plan.h"
#include "brgemm_bf16_dma256_edge.h"
#include "brgemm_bf16_dma256_images.h"
#include "brgemm_bf16_lw_launch.h"
#include "brgemm_f32_lw_kedge.h"
#include <set>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace tpp;

namespace {

// ---- the switches ------------------------------------------------------------------------------------------------------------------
enum { SW_D256E = 1, SW_ET = 2, SW_EK = 4, SW_EKB = 8, SW_EK8 = 16, SW_IMG = 32, SW_TAIL = 64, SW_HALVES = 128, SW_ALL = 255 };
const char *const SW_NAME[8] = {"dma256_edge", "edge_tiles", "edge_k", "edge_k_bf16", "edge_k8_bf16", "dma256_images", "tail_split", "halves"};
const int SW_F32 = SW_ET | SW_EK | SW_TAIL | SW_HALVES, SW_BF16 = SW_D256E | SW_ET | SW_EKB | SW_EK8 | SW_IMG;

// the refinements in the planner's precedence (the order of plan_gemm_call's blocks), and what each reads besides the descriptor, the call,
// the compute units and xsmm_hip_force_split
enum Ref { R_D256E, R_BF16_EDGE, R_BF16_KEDGE, R_K8, R_IMAGES, R_F32_EDGE, R_F32_KEDGE, R_TAIL, R_HALVES, R_NONE };
const char *const REF_NAME[10] = {"dma256_edge", "bf16_edge_tiles", "bf16_ragged_k", "half_step_k", "dma256_images",
                                  "f32_edge_tiles", "f32_ragged_k", "tail_split", "halves", "none"};
const int READS[9] = {SW_D256E, SW_ET, SW_EKB | SW_ET, SW_EK8 | SW_ET, SW_IMG, SW_ET, SW_EK | SW_ET, SW_TAIL, SW_HALVES};

// a context: the value each member of a set has, in the order of SW_NAME, and xsmm_hip_force_split
struct Ctx {
  const char *name;
  int value[8];
  int forced_split;
};
const Ctx CTX[6] = {
    {"rule", {1, 2, 1, 1, 1, 1, 1, 1}, -1},
    {"eligible", {2, 2, 1, 1, 1, 2, 2, 2}, -1},
    // tile-naming values: edge tiles 64x64 (bf16), f32 ragged k 64x32 + K4, bf16 ragged k 32x64, half steps 64x128
    {"forcing", {2, V_BF16_LW_64x64, V_F32_LW_64x32K2, V_BF16_LW_32x64, V_BF16_LW_64x128, 2, 2, 2}, 4},
    // ... edge tiles 32x32 + K4 (f32), f32 ragged k 64x64 + K2, bf16 ragged k 128x128, half steps 32x64
    {"forcing-f32", {2, V_F32_LW_32x32K4, V_F32_LW_64x64K2, V_BF16_LW_128x128, V_BF16_LW_32x64, 2, 2, 2}, 4},
    // the table only: "eligible" and "rule" under xsmm_hip_force_split(2)
    {"eligible-split2", {2, 2, 1, 1, 1, 2, 2, 2}, 2},
    {"rule-split2", {1, 2, 1, 1, 1, 1, 1, 1}, 2}};
const int N_SWEEP_CTX = 4;

GemmPlanEnv make_env(const Ctx &c, int set, int cus, bool strict) {
  GemmPlanEnv e{cus, strict, c.forced_split};
  auto v = [&](int i) { return set >> i & 1 ? c.value[i] : 0; };
  e.dma256_edge = v(0), e.edge_tiles = v(1), e.edge_k = v(2), e.edge_k_bf16 = v(3), e.edge_k8_bf16 = v(4), e.dma256_images = v(5), e.tail_split = v(6),
  e.halves = v(7);
  return e;
}

std::string set_name(int set) {
  std::string s;
  for (int i = 0; i < 8; ++i)
    if (set >> i & 1) s += (s.empty() ? "" : "+") + std::string(SW_NAME[i]);
  return s.empty() ? "{}" : s;
}

// ---- descriptors and calls -----------------------------------------------------------------------------------------------------------
struct Form {
  const char *name;
  int dtype, vnni_b, vf;
};
const Form F32F{"f32", DT_F32, 0, 0}, V2{"v2", DT_BF16, 1, 2}, FLAT{"flat", DT_BF16, 0, 0}, V4{"v4", DT_BF16, 1, 4};
const Form *const FORMS[4] = {&F32F, &V2, &FLAT, &V4};

struct Spec {
  const Form *f;
  int64_t m, n, k;
  const char *ep;  // b: beta 0, B: bias, r: relu
  int forced;
  int vc;
  // P packed; R wide rows on the 16-byte grid whatever m, n and k are; C ldc off the bf16 grid; B ldb and ldc off both grids; K the strided layout of
  // tests/dma256_images_worker.py Case for `br` batch elements; L the layout of tests/edge_tiles_worker.py layer_call for `br` batch elements
  char layout;
  int br;
};

GemmDesc make_desc(const Spec &s) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.dtype = s.f->dtype;
  d.m = s.m, d.n = s.n, d.k = s.k;
  const int64_t nb = s.br > 1 ? s.br : 1;
  d.lda = s.k, d.ldb = s.n, d.ldc = s.n, d.stride_a = s.m * s.k, d.stride_b = s.k * s.n;
  switch (s.layout) {
  case 'R': d.lda = (s.k + 7) / 8 * 8 + 8, d.ldb = (s.n + 7) / 8 * 8 + 8, d.ldc = (s.n + 7) / 8 * 8 + 16, d.stride_a = s.m * d.lda, d.stride_b = (s.k + 3) / 4 * 4 * d.ldb; break;
  case 'C': d.ldc = s.n + 4; break;
  case 'B': d.ldb = s.n + 2, d.ldc = s.n + 2, d.stride_b = s.k * d.ldb; break;
  case 'K': d.lda = nb * (s.k + 8) + 8, d.stride_a = s.k + 8, d.ldb = s.n + 8, d.ldc = s.n + 16, d.stride_b = (s.k + 4) * d.ldb; break;
  case 'L': d.lda = nb * s.k, d.stride_a = s.k, d.stride_b = s.k * d.ldb; break;
  default: break;
  }
  d.beta0 = strchr(s.ep, 'b') != nullptr;
  d.bias = strchr(s.ep, 'B') != nullptr;
  d.relu = strchr(s.ep, 'r') != nullptr;
  d.fused = d.bias || d.relu;
  d.vnni_b = s.f->vnni_b;
  d.vnni_factor = s.f->vf;
  d.vnni_c = s.vc;
  return d;
}

std::string desc_text(const Spec &s, const GemmDesc &d) {
  char buf[320];
  snprintf(buf, sizeof buf, "%s %ldx%ldx%ld ld%ld,%ld,%ld s%ld,%ld e%s f%d%s : v%d %s%s%s", s.f->name, (long)d.m, (long)d.n, (long)d.k, (long)d.lda, (long)d.ldb,
           (long)d.ldc, (long)d.stride_a, (long)d.stride_b, *s.ep ? s.ep : "-", s.forced, s.vc ? " vc" : "", d.variant, d.name, d.generic_forced ? " gf" : "",
           d.variant_forced ? " vf" : "");
  return buf;
}

// pointer alignments in bytes: A and B, C, the bias row
struct Call {
  int br, ab, c, d;
};
GemmAlign align_of(const Call &c) { return GemmAlign{c.ab >= 16, c.c >= 16, c.c >= 8, c.d >= 8, c.d >= 16}; }
std::string call_text(const Call &c) {
  char buf[64];
  snprintf(buf, sizeof buf, "br%d a%d/%d/%d", c.br, c.ab, c.c, c.d);
  return buf;
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
const char *launcher_name(GemmLauncher l) {
  static const char *const n[] = {"none", "invalid", "f32_fast", "f32_lw", "f32_lw16", "f32_lw_grouped", "f32_x6", "bf16_fast", "bf16_small32",
                                  "bf16_grouped64", "bf16_lw", "bf16_lw_grouped", "bf16_lw_quads", "generic"};
  return (int)l >= 0 && (int)l < 14 ? n[l] : "?";
}
std::string launch_text(const GemmLaunch &l) {
  char buf[320];
  int o = snprintf(buf, sizeof buf, "%s t%d s%d b%d", launcher_name(l.launcher), l.tile, l.split, l.b_kind);
  if (l.even) o += snprintf(buf + o, sizeof buf - o, " even");
  if (l.vec) o += snprintf(buf + o, sizeof buf - o, " vec");
  if (l.launcher == GL_GENERIC) o += snprintf(buf + o, sizeof buf - o, " g%d", (int)l.generic);
  if (l.tail_tiles || l.tail_split != 1) o += snprintf(buf + o, sizeof buf - o, " tail%dx%d", l.tail_tiles, l.tail_split);
  if (l.edge) o += snprintf(buf + o, sizeof buf - o, " edge");
  if (l.edge_k) o += snprintf(buf + o, sizeof buf - o, " edge_k");
  if (l.edge_k8) o += snprintf(buf + o, sizeof buf - o, " edge_k8");
  if (l.halves) o += snprintf(buf + o, sizeof buf - o, " halves");
  snprintf(buf + o, sizeof buf - o, " \"%s\"", l.text ? l.text : "(null)");
  return buf;
}
// field by field, the text included
bool same(const GemmLaunch &a, const GemmLaunch &b) {
  return a.launcher == b.launcher && a.tile == b.tile && a.split == b.split && a.b_kind == b.b_kind && a.even == b.even && a.vec == b.vec &&
         (a.launcher != GL_GENERIC || a.generic == b.generic) && a.tail_tiles == b.tail_tiles && a.tail_split == b.tail_split && a.edge == b.edge &&
         a.edge_k == b.edge_k && a.edge_k8 == b.edge_k8 && a.halves == b.halves && a.text && b.text && strcmp(a.text, b.text) == 0;
}
Ref refinement(const GemmLaunch &l) {
  if (l.launcher == GL_BF16_FAST && l.edge) return R_D256E;
  if (l.launcher == GL_BF16_LW && l.edge_k8) return R_K8;
  if (l.launcher == GL_BF16_LW && l.edge_k) return R_BF16_KEDGE;
  if (l.launcher == GL_BF16_LW && l.edge) return R_BF16_EDGE;
  if (l.launcher == GL_BF16_FAST && l.b_kind != 0) return R_IMAGES;
  if (l.launcher == GL_F32_LW && l.edge_k) return R_F32_KEDGE;
  if (l.launcher == GL_F32_LW && l.edge) return R_F32_EDGE;
  if (l.tail_tiles > 0) return R_TAIL;
  if (l.halves) return R_HALVES;
  return R_NONE;
}

// ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------
long long g_decisions = 0, g_fail = 0, g_fail_kind[8];
long long g_reached[9][3]; // per refinement and B image (f32 refinements: column 0)
std::set<std::string> g_refused;
std::vector<std::string> g_refused_lines;

GemmLaunch plan(const GemmDesc &d, const Call &c, const GemmPlanEnv &e) {
  ++g_decisions;
  return plan_gemm_call(d, c.br, align_of(c), e);
}

void fail(int kind, const char *check, const std::string &desc, const Call &c, const Ctx &ctx, int cus, int set, const std::string &what) {
  ++g_fail;
  if (++g_fail_kind[kind] <= 25)
    printf("FAIL %s: %s | %s | %s cus%d %s | %s\n", check, desc.c_str(), call_text(c).c_str(), ctx.name, cus, set_name(set).c_str(), what.c_str());
}

// ---- d: what the launchers refuse, restated where a header does not hold it -----------------------------------------------------------
// the f32 loader-wave tiles as launch_f32_lw / launch_f32_lw_edge / launch_f32_lw_kedge number them: 1 = 64x64 + K2, 2 = 64x32 + K4, 3 = 32x32 + K4, 4 = 128x64
const int F32_BM[5] = {64, 64, 64, 32, 128}, F32_BN[5] = {64, 64, 32, 32, 64};

const char *launcher_refuses(const GemmDesc &d, const Call &c, const GemmLaunch &l) {
  const GemmAlign al = align_of(c);
  const int br = c.br < 0 ? 0 : c.br;
  if (l.launcher == GL_BF16_LW) {
    // brgemm_bf16_lw.hip launch_bf16_lw: blw_launch_ok, then the instance of blw_sup's chunks per barrier (lines 1174-1179, 1198-1199)
    const int mode = l.edge_k8 ? BLW_KEDGE8 : l.edge_k ? BLW_KEDGE : l.edge ? BLW_EDGE : BLW_LAYER;
    BlwShape h{false, (int)d.m, (int)d.n, 1, 0, {}, {}};
    h.k[0] = (int)d.k, h.br[0] = br;
    if (!blw_launch_ok(mode, l.tile, l.b_kind, h)) return "blw_launch_ok";
    const int sup = blw_one_chunk(mode) || !blw_tile_sup2(l.tile) || ((br * (d.k / 64)) & 1) ? 1 : 2;
    if (!blw_instance_exists(mode, false, l.tile, l.b_kind, sup)) return "blw_instance_exists";
    return nullptr;
  }
  if (l.launcher == GL_BF16_FAST && (l.edge || l.b_kind != 0)) {
    if (l.tile != 2) return "the 256x256 tile only"; // brgemm_f32.hip run_gemm_launch, GL_BF16_FAST
    // brgemm_bf16_dma256_edge.hip launch_bf16_dma256_edge lines 40-44 / brgemm_bf16_dma256.hip launch_bf16_dma256_image lines 39-42
    if (!d256_image_ok(l.b_kind) || d.k <= 0 || d.k % D256_BK || br < 1) return "image, k % 32 or the batch";
    if (l.edge ? !d256e_extent_ok(d.m) || !d256e_extent_ok(d.n) || d.n % 8 || d.ldb < d.n : d.m <= 0 || d.n <= 0 || d.m % D256_BM || d.n % D256_BN)
      return "m or n";
    if (!d256_b_ldb_ok(l.b_kind, d.ldb) || d.lda < d.k || d.ldc < d.n || ((d.lda | d.ldc | d.stride_a | d.stride_b) & 7) || d.lda >= (1 << 22) || d.ldc >= (1 << 22))
      return "a leading dimension or stride";
    if (!al.ab16 || !al.c16 || (d.bias && !al.d8) || d.vnni_c) return "an alignment or a VNNI C";
    return nullptr;
  }
  if (l.launcher == GL_F32_LW && (l.edge || l.edge_k)) {
    // brgemm_f32_lw.hip launch_lw_edge_t lines 684-687, launch_lw_kedge_t lines 695-698; tiles 1 .. 4 (launch_f32_lw_edge lines 762-769, _kedge 774-781)
    if (l.tile < 1 || l.tile > 4) return "tile";
    const int bm = F32_BM[l.tile], bn = F32_BN[l.tile];
    if (d.m < bm || d.n < bn || (d.n & 3) || br < 1) return "m, n or the batch";
    if (l.edge_k ? !kedge_k_ok(d.k) : d.k <= 0 || d.k % 64 != 0) return "k";
    if ((d.m + bm - 1) / bm > 65535 || (d.n + bn - 1) / bn > 65535) return "grid";
    return nullptr;
  }
  if (l.launcher == GL_F32_LW && l.tail_tiles > 0) {
    // brgemm_f32_lw.hip launch_lw_tail_t line 671; tiles 1 .. 3 (launch_f32_lw_tail lines 751-757)
    if (l.tile < 1 || l.tile > 3) return "tile";
    const int bm = F32_BM[l.tile], bn = F32_BN[l.tile];
    const long long tiles = (long long)(d.m / bm) * (d.n / bn), body = tiles - l.tail_tiles;
    if (d.m % bm || d.n % bn || body <= 0 || l.tail_split < 2 || l.tail_split > 16 || body + (long long)l.tail_tiles * l.tail_split > 0x7fffffffLL) return "tail";
    return nullptr;
  }
  if (l.halves) {
    // brgemm_f32.hip launch_gemm: GL_F32_LW, tile 1; brgemm_f32_lw.hip launch_f32_lw_halves line 712
    if (l.launcher != GL_F32_LW || l.tile != 1) return "launcher or tile";
    if (d.m <= 0 || d.n <= 0 || d.m % 64 || d.n % 64 || d.k <= 0 || d.k % 64) return "halves";
    return nullptr;
  }
  if (l.split > 1 && (l.launcher == GL_F32_LW || l.launcher == GL_F32_LW16)) {
    // brgemm_f32_lw.hip launch_f32_lw_split lines 740-746: the K-split tiles 1 .. 3 (GL_F32_LW16: tile 3); at most SPLIT_MAX workgroups
    const int tile = l.launcher == GL_F32_LW ? l.tile : 3;
    if (tile < 1 || tile > 3 || l.split > 16) return "split";
  }
  return nullptr;
}

// ---- c: what every launch keeps ---------------------------------------------------------------------------------------------------------
const char *invariant_broken(const GemmDesc &d, const Call &c, const GemmPlanEnv &env, const GemmLaunch &l) {
  if (!l.text) return "no text";
  const GemmAlign al = align_of(c);
  const Ref r = refinement(l);
  if (l.edge_k && l.edge_k8) return "edge_k and edge_k8";
  if ((int)l.edge + (int)l.edge_k + (int)l.edge_k8 > 1) return "more than one of edge, edge_k, edge_k8";
  if ((l.edge || l.edge_k) && l.launcher != GL_BF16_LW && l.launcher != GL_F32_LW && !(l.launcher == GL_BF16_FAST && l.edge)) return "an edge flag on another launcher";
  if (l.edge_k8 && l.launcher != GL_BF16_LW) return "edge_k8 on another launcher";
  if (l.launcher == GL_BF16_LW && l.edge_k && !(d.k >= 64 && d.k % 16 == 0 && d.k % 64 != 0)) return "bf16 edge_k: k";
  if (l.launcher == GL_F32_LW && l.edge_k && !(d.k >= 64 && d.k % 8 == 0 && d.k % 64 != 0)) return "f32 edge_k: k";
  if (l.edge_k8 && !(d.k >= 64 && d.k % 16 == 8)) return "edge_k8: k";
  if (l.launcher == GL_BF16_LW && (l.edge || l.edge_k || l.edge_k8)) {
    int bm, bn;
    if (l.tile < 0 || l.tile > 3) return "ragged bf16 launch: tile";
    blw_tile_dims(l.tile, &bm, &bn);
    if (d.m < bm || d.n < bn || d.n % 8 != 0) return "ragged bf16 launch: m >= BM, n >= BN, n % 8";
    if (l.edge && d.k % 64 != 0) return "bf16 edge tiles: k";
  }
  if (l.launcher == GL_BF16_FAST && l.edge && !(l.tile == 2 && d.m >= 256 && d.n >= 256 && (d.m % 256 || d.n % 256) && d.k % 32 == 0 && d.n % 8 == 0))
    return "dma256 edge: shape";
  if (l.launcher == GL_BF16_FAST && !l.edge && l.b_kind != 0 && !(l.tile == 2 && d.m % 256 == 0 && d.n % 256 == 0 && (l.b_kind == 2 || l.b_kind == 4)))
    return "dma256 images: shape or image";
  if ((l.launcher == GL_BF16_FAST || l.launcher == GL_BF16_LW) && l.b_kind != (d.vnni_b ? (d.vnni_factor == 4 ? 4 : 0) : 2)) return "B image";
  if (l.halves && !(l.launcher == GL_F32_LW && l.tile == 1 && l.split == 1 && l.tail_tiles == 0)) return "halves: tile 1, split 1, no tail";
  if (l.tail_tiles > 0 && !(l.split == 1 && l.launcher == GL_F32_LW && l.tail_split >= 2)) return "tail split: split 1";
  if (l.tail_tiles == 0 && l.tail_split != 1) return "tail_split without tail tiles";
  if (l.split < 1) return "split < 1";
  // a forced variant, the forced generic kernel, a VNNI C and an empty batch: none of the seven refinements that leave the dispatched kernel.
  // (Split, tail split and halves act on the K-split f32 tile a call was DISPATCHED on, forced or not - gemm_plan.cpp choose_f32_halves "a forced
  // tile only", tests/test_f32_halves_gpu.py, tests/test_tail_split_gpu.py - and halves keeps an empty batch, as launch_f32_lw does.)
  if (r <= R_F32_KEDGE && (d.variant_forced || d.generic_forced || d.vnni_c || c.br < 1)) return "a refinement of a forced, VNNI-C or empty call";
  if (r != R_NONE && (d.generic_forced || d.vnni_c)) return "a refinement of the forced generic kernel";
  if (r == R_TAIL && c.br < 1) return "a tail split of an empty batch";
  if (l.split > 1 && c.br < 1) return "a split of an empty batch";
  // ragged k on a tile that does not divide m and n: only with the edge tiles of that type on as well; and the text says what the launch is
  const bool ragged_k = r == R_BF16_KEDGE || r == R_K8 || r == R_F32_KEDGE;
  bool mn_ragged = false;
  if (r == R_BF16_EDGE || r == R_BF16_KEDGE || r == R_K8) {
    int bm, bn;
    blw_tile_dims(l.tile, &bm, &bn);
    mn_ragged = d.m % bm != 0 || d.n % bn != 0;
    const bool edge_on = env.edge_tiles == 2 || (env.edge_tiles >= V_BF16_LW_32x64 && env.edge_tiles <= V_BF16_LW_128x128);
    if (mn_ragged && !edge_on) return "a bf16 tile that does not divide m and n without the bf16 edge tiles";
    if (r == R_BF16_EDGE && !mn_ragged) return "bf16 edge tiles on a tile that divides m and n";
  }
  if (r == R_F32_EDGE || r == R_F32_KEDGE) {
    if (l.tile < 1 || l.tile > 4) return "ragged f32 launch: tile";
    mn_ragged = d.m % F32_BM[l.tile] != 0 || d.n % F32_BN[l.tile] != 0;
    const int et = env.edge_tiles;
    const bool edge_on = et == 1 || et == 2 || et == V_F32_LW_64x64K2 || et == V_F32_LW_64x32K2 || et == V_F32_LW_32x32K4 || et == V_F32_LW_128x64;
    if (mn_ragged && !edge_on) return "an f32 tile that does not divide m and n without the f32 edge tiles";
    if (d.m < F32_BM[l.tile] || d.n < F32_BN[l.tile] || d.n % 4 != 0) return "ragged f32 launch: m >= BM, n >= BN, n % 4";
    if (r == R_F32_EDGE && d.k % 64 != 0) return "f32 edge tiles: k";
  }
  if (r <= R_F32_KEDGE) {
    const bool says_edge = strstr(l.text, "edge tiles") != nullptr, says_k = strstr(l.text, "ragged k") != nullptr, says_half = strstr(l.text, "half step") != nullptr;
    if (says_edge != (l.edge || (ragged_k && mn_ragged)) || says_k != ragged_k || says_half != (r == R_K8)) return "the text does not say what the launch is";
    if (r < R_F32_EDGE && ((strstr(l.text, "_flatb<") != nullptr) != (l.b_kind == 2) || (strstr(l.text, "_vnni4<") != nullptr) != (l.b_kind == 4))) return "the text names another B image";
    if ((r == R_D256E || r == R_IMAGES) != (strstr(l.text, "<256x256>") != nullptr)) return "the text names another tile";
  }
  if ((r == R_TAIL) != (strstr(l.text, "tail split") != nullptr)) return "the text and the tail split disagree";
  // 16-byte pieces: what the loader-wave kernels and the 256x256 tile ask of pointers, leading dimensions and strides (bf16: 16-byte stores of C, 8-byte
  // reads of the bias row, LDS-DMA rows of A and of each B image; f32: 16-byte pieces of A, B, C and the bias row)
  if (r <= R_IMAGES) {
    if (!al.ab16 || !al.c16 || (d.bias && !al.d8)) return "a bf16 refinement of a misaligned call";
    if (((d.lda | d.ldc | d.stride_a | d.stride_b) & 7) || d.ldb % (l.b_kind == 0 ? 4 : l.b_kind == 2 ? 8 : 2) != 0) return "a bf16 refinement off the 16-byte grid";
  }
  if (r == R_F32_EDGE || r == R_F32_KEDGE) {
    if (!al.ab16 || !al.c16 || (d.bias && !al.d16)) return "an f32 refinement of a misaligned call";
    if (((d.lda | d.ldb | d.stride_a | d.stride_b) & 3) || d.ldc % 4 != 0) return "an f32 refinement off the 16-byte grid";
  }
  return nullptr;
}

// ---- e: the refusal cascade of brgemm_f32.hip launch_gemm ------------------------------------------------------------------------------
// block order: 0 dma256 edge, 1 dma256 images, 2 half-step k, 3 bf16 ragged k, 4 f32 ragged k (any launch with edge_k), 5 edge tiles (any launch with
// edge); each refuses by zeroing ONE mode and planning again, and control goes on BELOW it. 6 split, 7 tail split, 8 halves fall back without planning.
int cascade_block(const GemmLaunch &p, int from) {
  for (int b = from; b < 6; ++b) {
    const bool hit = b == 0 ? p.launcher == GL_BF16_FAST && p.edge : b == 1 ? p.launcher == GL_BF16_FAST && p.b_kind != 0 : b == 2 ? p.edge_k8 && p.launcher == GL_BF16_LW
                     : b == 3 ? p.edge_k && p.launcher == GL_BF16_LW : b == 4 ? p.edge_k : p.edge;
    if (hit) return b;
  }
  return 6;
}
// returns nullptr or what went wrong; *steps: the refusals walked
const char *cascade(const GemmDesc &d, const Call &c, GemmPlanEnv env, GemmLaunch p, int *steps, std::string *trail) {
  int pos = 0;
  *steps = 0;
  while (true) {
    const int b = cascade_block(p, pos);
    if (b == 6) break;
    if (++*steps > 9) return "more than nine steps";
    *trail += " > " + launch_text(p);
    (b == 0 ? env.dma256_edge : b == 1 ? env.dma256_images : b == 2 ? env.edge_k8_bf16 : b == 3 ? env.edge_k_bf16 : b == 4 ? env.edge_k : env.edge_tiles) = 0;
    p = plan(d, c, env);
    pos = b + 1;
    // a refinement of a block launch_gemm has already passed would reach run_gemm_launch at the bottom without its fallback or counter
    if (cascade_block(p, 0) < pos) return *trail += " > " + launch_text(p), "the re-plan carries a refinement of an earlier block";
  }
  // below the blocks: a split launch that is refused runs unsplit, then a tail split, then halves, then the plain launch
  if (p.split > 1 && (p.launcher == GL_F32_LW || p.launcher == GL_F32_LW16)) {
    ++*steps;
    if (p.tail_tiles > 0 || p.halves) return "a split launch with a tail or halves behind it";
  }
  if (p.tail_tiles > 0) {
    ++*steps;
    if (p.launcher != GL_F32_LW) return "a tail split on another launcher";
    if (p.halves) return "a tail split with halves behind it";
    p.tail_tiles = 0, p.tail_split = 1;
  }
  if (p.halves) {
    ++*steps;
    if (p.launcher != GL_F32_LW || p.tile != 1) return "halves on another launcher or tile";
    p.halves = false;
  }
  if (*steps > 9) return "more than nine steps";
  if (p.edge || p.edge_k || p.edge_k8 || p.tail_tiles > 0 || p.halves || (p.launcher == GL_BF16_FAST && p.b_kind != 0)) return "a refinement flag at the bottom";
  return nullptr;
}

// ---- one descriptor and call under every set of every context ------------------------------------------------------------------------
void check_call(const GemmDesc &d, const std::string &dt, const Call &c, int cus, bool strict) {
  static GemmLaunch P[256];
  for (int ci = 0; ci < N_SWEEP_CTX; ++ci) {
    const Ctx &ctx = CTX[ci];
    for (int S = 0; S < 256; ++S) P[S] = plan(d, c, make_env(ctx, S, cus, strict));
    for (int S = 0; S < 256; ++S) {
      const GemmLaunch &l = P[S];
      const Ref r = refinement(l);
      // b: one precedence list - the first refinement that takes the call under ITS OWN read set wins, and the launch is that launch
      int winner = R_NONE;
      for (int y = 0; y < 9 && winner == R_NONE; ++y)
        if (refinement(P[S & READS[y]]) == y) winner = y;
      const GemmLaunch &want = winner == R_NONE ? P[0] : P[S & READS[winner]];
      if (!same(l, want))
        fail(1, "b precedence", dt, c, ctx, cus, S, "got " + launch_text(l) + " want (" + REF_NAME[winner] + ") " + launch_text(want));
      if (r != R_NONE && !same(l, P[S & READS[r]])) fail(1, "b read set", dt, c, ctx, cus, S, "got " + launch_text(l) + " under its read set " + launch_text(P[S & READS[r]]));
      if (r == R_NONE && !same(l, P[0])) fail(1, "b no refinement", dt, c, ctx, cus, S, "got " + launch_text(l) + " under {} " + launch_text(P[0]));
      if (!same(l, P[S & (d.dtype == DT_F32 ? SW_F32 : SW_BF16)])) fail(1, "b other type's switch", dt, c, ctx, cus, S, launch_text(l));
      if ((r == R_K8 && !same(l, P[S & ~SW_EKB])) || (r == R_BF16_KEDGE && !same(l, P[S & ~SW_EK8]))) fail(1, "b ragged-k switches", dt, c, ctx, cus, S, launch_text(l));
      // c
      if (const char *why = invariant_broken(d, c, make_env(ctx, S, cus, strict), l)) fail(2, "c invariant", dt, c, ctx, cus, S, std::string(why) + ": " + launch_text(l));
      // d
      if (const char *why = launcher_refuses(d, c, l)) {
        const std::string key = dt + " | " + call_text(c) + " | " + launch_text(l);
        if (g_refused.insert(key).second) g_refused_lines.push_back("REFUSED " + key + " | first under " + ctx.name + " " + set_name(S) + " | " + why);
      }
      if (r != R_NONE) ++g_reached[r][d.dtype == DT_F32 ? 0 : l.b_kind / 2];
    }
    // e: from every distinct refined launch
    for (int S = 0; S < 256; ++S) {
      if (refinement(P[S]) == R_NONE && P[S].split <= 1) continue;
      int steps = 0;
      std::string trail;
      if (const char *why = cascade(d, c, make_env(ctx, S, cus, strict), P[S], &steps, &trail)) fail(4, "e cascade", dt, c, ctx, cus, S, std::string(why) + ":" + trail);
    }
    // c, last line: strict mode changes nothing but split, tail split and halves
    static const int SETS[10] = {0, 1, 2, 4, 8, 16, 32, 64, 128, 255};
    for (int S : SETS) {
      const GemmLaunch o = plan(d, c, make_env(ctx, S, cus, !strict));
      const GemmLaunch &l = P[S];
      const bool soft = l.split > 1 || o.split > 1 || l.tail_tiles > 0 || o.tail_tiles > 0 || l.halves || o.halves;
      if (soft ? l.launcher != o.launcher || l.tile != o.tile || l.b_kind != o.b_kind || l.edge != o.edge || l.edge_k != o.edge_k || l.edge_k8 != o.edge_k8 : !same(l, o))
        fail(2, "c strict", dt, c, ctx, cus, S, launch_text(l) + " other strict setting " + launch_text(o));
    }
  }
}

long long g_descs = 0;
void check_desc(const Spec &s, const std::vector<Call> &calls, int cus, bool strict) {
  GemmDesc d = make_desc(s);
  plan_gemm(d, s.forced, GemmPlanEnv{cus, strict, -1});
  const std::string dt = desc_text(s, d);
  ++g_descs;
  // a: dispatch reads no single-call switch - every set of "eligible", and the full set and xsmm_hip_force_split of the other contexts
  for (int ci = 0; ci < N_SWEEP_CTX; ++ci)
    for (int S = ci == 1 ? 0 : 255; S < 256; ++S) {
      GemmDesc e = make_desc(s);
      const bool ok = plan_gemm(e, s.forced, make_env(CTX[ci], S, cus, strict));
      if (!ok || e.variant != d.variant || strcmp(e.name, d.name) || e.generic_forced != d.generic_forced || e.variant_forced != d.variant_forced)
        fail(0, "a dispatch", dt, Call{0, 16, 16, 16}, CTX[ci], cus, S, std::string("variant ") + std::to_string(e.variant) + " " + e.name);
    }
  for (const Call &c : calls) check_call(d, dt, c, cus, strict);
}

int sweep(int cus, bool strict, bool quick) {
  static const int64_t MS[] = {32, 40, 64, 128, 248, 256, 264, 520, 544, 1000, 1024, 4000, 4100};
  static const int64_t NS[] = {36, 64, 72, 128, 256, 260, 264, 504, 1000, 1024, 4096};
  static const int64_t KS[] = {32, 64, 72, 80, 96, 200, 224, 400, 784, 1000, 1024, 1040};
  // the whole shape lattice: beta 0 + bias + relu, packed, aligned, one batch element and thirteen (past the ragged-k gate br * k < 1024)
  const std::vector<Call> plain = {{1, 16, 16, 16}, {13, 16, 16, 16}};
  long long lattice_index = 0;
  for (const Form *f : FORMS)
    for (int64_t m : MS)
      for (int64_t n : NS)
        for (int64_t k : KS)
          if (!quick || lattice_index++ % 8 == 0) check_desc(Spec{f, m, n, k, "bBr", -1, 0, 'P', 1}, plain, cus, strict);
  // a sub-lattice that still crosses every term of every block, under everything else a call can differ in
  // (n = 70 and 260 with rows on the 16-byte grid: the n % 4 and n % 8 terms alone)
  static const int64_t M2[] = {40, 64, 264, 1024}, N2[] = {36, 70, 72, 256, 260, 264, 1000}, K2[] = {64, 72, 80, 1024};
  const std::vector<Call> batches = {{0, 16, 16, 16}, {2, 16, 16, 16}, {16, 16, 16, 16}}, one = {{13, 16, 16, 16}};
  std::vector<Call> aligns;
  for (int br : {13})
    for (const Call &a : {Call{0, 8, 16, 16}, Call{0, 16, 8, 16}, Call{0, 16, 4, 16}, Call{0, 16, 16, 4}, Call{0, 16, 16, 8}}) aligns.push_back(Call{br, a.ab, a.c, a.d});
  static const int FORCED[4][5] = {{V_F32_LW_64x64K2, V_F32_LW_32x32K4, V_F32_LW16_32x16, V_GENERIC, -2},
                                   {V_BF16_DMA256, V_BF16_SMALL32, V_BF16_LW_64x64, V_GENERIC, -2},
                                   {V_BF16_LWF_64x64, V_BF16_LWF_128x128, V_GENERIC, -2, -2},
                                   {V_BF16_LW4_32x64, V_BF16_LW4_128x128, V_GENERIC, -2, -2}};
  for (int fi = 0; fi < 4; ++fi)
    for (int64_t m : M2)
      for (int64_t n : N2)
        for (int64_t k : K2) {
          const Form *f = FORMS[fi];
          check_desc(Spec{f, m, n, k, "bBr", -1, 0, 'P', 1}, batches, cus, strict);
          check_desc(Spec{f, m, n, k, "bBr", -1, 0, 'P', 1}, aligns, cus, strict);
          for (const char *ep : {"b", "B", ""}) check_desc(Spec{f, m, n, k, ep, -1, 0, 'P', 1}, one, cus, strict);
          check_desc(Spec{f, m, n, k, "bBr", -1, 1, 'P', 1}, plain, cus, strict); // a VNNI C
          for (int j = 0; j < 5 && FORCED[fi][j] != -2; ++j) check_desc(Spec{f, m, n, k, "bBr", FORCED[fi][j], 0, 'P', 1}, plain, cus, strict);
          for (char layout : {'R', 'C', 'B'}) check_desc(Spec{f, m, n, k, "bBr", -1, 0, layout, 1}, one, cus, strict);
        }
  for (const std::string &l : g_refused_lines) printf("%s\n", l.c_str());
  printf("planner accepts, launcher refuses: %zu\n", g_refused_lines.size());
  printf("refinements reached:");
  bool covered = true;
  for (int r = 0; r < 9; ++r) {
    const bool f32 = r >= R_F32_EDGE;
    if (f32) printf(" %s %lld", REF_NAME[r], g_reached[r][0]);
    else printf(" %s %lld/%lld/%lld", REF_NAME[r], g_reached[r][0], g_reached[r][1], g_reached[r][2]);
    // (the VNNI-2 image of the 256x256 tile is the dispatched kernel itself, brgemm_bf16_dma<256x256>: xsmm_hip_set_dma256_images has two images)
    for (int b = 0; b < (f32 ? 1 : 3); ++b)
      if (g_reached[r][b] == 0 && !(r == R_IMAGES && b == 0)) covered = false;
  }
  printf("\n");
  if (!covered && !quick) printf("FAIL coverage: a refinement was never reached with a B image it has\n"), ++g_fail;
  printf("%d compute units, strict %d: %lld descriptors, %lld decisions, %lld FAIL\n", cus, (int)strict, g_descs, g_decisions, g_fail);
  if (g_fail == 0) printf("OK\n");
  return g_fail ? 1 : 0;
}

// ---- f: the golden table -----------------------------------------------------------------------------------------------------------------
struct Row {
  const char *label;
  Spec s;
  Call c;
  bool split2; // also under "eligible-split2" and "rule-split2"
};

int table() {
  const Call A16{1, 16, 16, 16};
  auto at = [](int br, int ab = 16, int c = 16, int d = 16) { return Call{br, ab, c, d}; };
  std::vector<Row> rows;
  auto add = [&](const char *label, const Form &f, int64_t m, int64_t n, int64_t k, Call c, const char *ep = "bBr", char layout = 'K', int forced = -1, int vc = 0,
                 bool split2 = false) { rows.push_back(Row{label, Spec{&f, m, n, k, ep, forced, vc, layout, c.br}, c, split2}); };
  // the rows tests/test_call_switches_gpu.py runs (tests/call_switches_worker.py ROWS, by label): bf16 in the strided layout of Case, f32 in layer_call's
  const Form *img[3] = {&V2, &FLAT, &V4};
  static const char *const tag[3] = {"v2", "flat", "v4"};
  static std::vector<std::string> labels; // (kept alive: Row holds pointers)
  labels.reserve(256);
  auto lab = [&](const std::string &s) { return labels.push_back(s), labels.back().c_str(); };
  for (int i = 0; i < 3; ++i) {
    add(lab(std::string("gpu:d256e-264x256x32-") + tag[i]), *img[i], 264, 256, 32, A16);
    add(lab(std::string("gpu:d256e-256x264x96-") + tag[i]), *img[i], 256, 264, 96, A16);
    add(lab(std::string("gpu:k8-fallthrough-264x264x72-") + tag[i]), *img[i], 264, 264, 72, A16);
    add(lab(std::string("gpu:bf16-edge-40x72x64-") + tag[i]), *img[i], 40, 72, 64, A16);
    add(lab(std::string("gpu:k8-64x64x72-") + tag[i]), *img[i], 64, 64, 72, A16);
    add(lab(std::string("gpu:bf16-both-40x72x72-") + tag[i]), *img[i], 40, 72, 72, A16);
    add(lab(std::string("gpu:bf16-both16-40x72x80-") + tag[i]), *img[i], 40, 72, 80, A16);
  }
  add("gpu:kedge-64x64x80-flat", FLAT, 64, 64, 80, A16);
  add("gpu:kedge-64x64x80-v4", V4, 64, 64, 80, A16);
  add("gpu:kedge-64x64x80-v2-br13", V2, 64, 64, 80, at(13));
  add("gpu:kedge-gated-64x64x80-v2-br1", V2, 64, 64, 80, A16);
  add("gpu:images-256x256x64-flat", FLAT, 256, 256, 64, A16);
  add("gpu:images-256x256x64-v4", V4, 256, 256, 64, A16);
  add("gpu:f32-edge-40x36x64", F32F, 40, 36, 64, A16, "bBr", 'L');
  add("gpu:f32-kedge-64x64x72", F32F, 64, 64, 72, A16, "bBr", 'L');
  add("gpu:f32-both-40x36x72", F32F, 40, 36, 72, A16, "bBr", 'L');
  add("gpu:halves-64x64x64-f6", F32F, 64, 64, 64, A16, "bBr", 'L', V_F32_LW_64x64K2);
  add("gpu:split-64x128x64-f6-br4", F32F, 64, 128, 64, at(4), "bBr", 'L', V_F32_LW_64x64K2, 0, true);
  add("gpu:stays-128x128x64-f32", F32F, 128, 128, 64, A16, "bBr", 'L');
  add("gpu:stays-128x128x64-v2", V2, 128, 128, 64, A16);
  add("gpu:stays-128x128x64-flat", FLAT, 128, 128, 64, A16);
  add("gpu:stays-forced-256x256x64-flat-f25", FLAT, 256, 256, 64, A16, "bBr", 'K', V_BF16_LWF_64x64);
  add("gpu:stays-forced-40x36x64-f32-f8", F32F, 40, 36, 64, A16, "bBr", 'L', V_GENERIC);
  add("gpu:stays-vc-264x256x32-v2", V2, 264, 256, 32, A16, "Br", 'L', -1, 1);
  add("gpu:stays-c8-264x256x32-v2", V2, 264, 256, 32, at(1, 16, 8, 16));
  add("gpu:stays-c8-40x36x64-f32", F32F, 40, 36, 64, at(1, 16, 8, 16), "bBr", 'L');
  // beta 1 without bias or relu: the same launches (the planner reads the bias for its alignment only)
  add("plain-264x256x32-flat", FLAT, 264, 256, 32, A16, "");
  add("plain-40x36x72-f32", F32F, 40, 36, 72, A16, "", 'L');
  // the tail split of tests/test_tail_split_gpu.py at each compute-unit count: 16 x (CUs / 16 + 1) tiles of 32x32 + K4
  add("tail-512x160-f9-br4", F32F, 512, 160, 64, at(4), "bBr", 'L', V_F32_LW_32x32K4);
  add("tail-512x544-f9-br4", F32F, 512, 544, 64, at(4), "bBr", 'L', V_F32_LW_32x32K4);
  add("tail-512x544-f9-br64", F32F, 512, 544, 64, at(64), "bBr", 'L', V_F32_LW_32x32K4);
  add("tail-512x640-f9-br4", F32F, 512, 640, 64, at(4), "bBr", 'L', V_F32_LW_32x32K4);
  // large layers, packed: the rules (mode 1) and their neighbours
  for (int i = 0; i < 3; ++i) {
    add(lab(std::string("d256e-rule-4000x4096x1024-") + tag[i]), *img[i], 4000, 4096, 1024, A16, "bBr", 'P');
    add(lab(std::string("d256e-gate-4100x4096x1024-") + tag[i]), *img[i], 4100, 4096, 1024, A16, "bBr", 'P');
    add(lab(std::string("d256e-k96-4000x4096x96-") + tag[i]), *img[i], 4000, 4096, 96, A16, "bBr", 'P');
    add(lab(std::string("images-4096x4096x1024-") + tag[i]), *img[i], 4096, 4096, 1024, A16, "bBr", 'P');
    add(lab(std::string("images-2048x2048x1024-") + tag[i]), *img[i], 2048, 2048, 1024, A16, "bBr", 'P');
    add(lab(std::string("ragged-1000x1000x1000-") + tag[i]), *img[i], 1000, 1000, 1000, A16, "bBr", 'P');
    add(lab(std::string("ragged-1000x1000x1024-") + tag[i]), *img[i], 1000, 1000, 1024, A16, "bBr", 'P');
    add(lab(std::string("ragged-1024x1024x400-") + tag[i]), *img[i], 1024, 1024, 400, A16, "bBr", 'P');
    add(lab(std::string("ragged-1024x1024x200-") + tag[i]), *img[i], 1024, 1024, 200, A16, "bBr", 'P');
  }
  add("gate-256x1024x400-v2-br1", V2, 256, 1024, 400, A16, "bBr", 'P');
  add("gate-256x1024x400-v2-br4", V2, 256, 1024, 400, at(4), "bBr", 'P');
  add("gate-128x1024x200-v2-br1", V2, 128, 1024, 200, A16, "bBr", 'P');
  add("f32-1000x1000x1024", F32F, 1000, 1000, 1024, A16, "bBr", 'P');
  add("f32-1000x1000x1000", F32F, 1000, 1000, 1000, A16, "bBr", 'P');
  add("f32-1024x1024x1000", F32F, 1024, 1024, 1000, A16, "bBr", 'P');
  add("f32-halves-1024x1024x1024", F32F, 1024, 1024, 1024, A16, "bBr", 'P');
  add("f32-halves-512x512x1024", F32F, 512, 512, 1024, A16, "bBr", 'P');
  add("f32-tail-1024x2560x64-br16", F32F, 1024, 2560, 64, at(16), "bBr", 'P', -1, 0, true);
  add("f32-tail-1024x1536x64-br16-f6", F32F, 1024, 1536, 64, at(16), "bBr", 'P', V_F32_LW_64x64K2, 0, true);
  add("f32-split-128x1024x64-br64", F32F, 128, 1024, 64, at(64), "bBr", 'P', -1, 0, true);
  add("f32-empty-1024x1024x64-br0-f6", F32F, 1024, 1024, 64, at(0), "bBr", 'P', V_F32_LW_64x64K2);
  add("empty-264x256x32-flat-br0", FLAT, 264, 256, 32, at(0));
  add("unaligned-264x256x32-v4-ab8", V4, 264, 256, 32, at(1, 8, 16, 16));
  add("bias4-264x256x32-flat", FLAT, 264, 256, 32, at(1, 16, 16, 4));
  add("bias8-40x36x64-f32", F32F, 40, 36, 64, at(1, 16, 16, 8), "bBr", 'L');
  add("offgrid-264x256x32-flat-ldc", FLAT, 264, 256, 32, A16, "bBr", 'C');
  add("n260-264x260x64-v2", V2, 264, 260, 64, A16, "bBr", 'P');
  printf("# <label> | <descriptor> | <call> | <context> cus<compute units that give this row> | {} <launch> | <switch> <launch, - = as {}> x 8 | all <launch>\n");
  int fails = 0;
  for (const Row &r : rows)
    for (int ci : {0, 1, 2, 4, 5}) {
      if (ci >= 4 && !r.split2) continue;
      const Ctx &ctx = CTX[ci];
      static const int CUS[3] = {64, 256, 304};
      std::string head[3], body[3];
      for (int q = 0; q < 3; ++q) {
        const int cus = CUS[q];
        GemmDesc d = make_desc(r.s);
        plan_gemm(d, r.s.forced, GemmPlanEnv{cus, false, -1});
        const GemmLaunch off = plan(d, r.c, make_env(ctx, 0, cus, false));
        head[q] = std::string(r.label) + " | " + desc_text(r.s, d) + " | " + call_text(r.c) + " | " + ctx.name;
        body[q] = " | {} " + launch_text(off);
        for (int i = 0; i < 8; ++i) {
          const GemmLaunch l = plan(d, r.c, make_env(ctx, 1 << i, cus, false));
          body[q] += std::string(" | ") + SW_NAME[i] + " " + (same(l, off) ? "-" : launch_text(l));
        }
        const GemmLaunch all = plan(d, r.c, make_env(ctx, SW_ALL, cus, false));
        body[q] += " | all " + launch_text(all);
        if (launcher_refuses(d, r.c, all)) ++fails;
      }
      bool done[3] = {false, false, false};
      for (int q = 0; q < 3; ++q) {
        if (done[q]) continue;
        std::string cus = " cus" + std::to_string(CUS[q]);
        for (int p = q + 1; p < 3; ++p)
          if (head[p] == head[q] && body[p] == body[q]) cus += "," + std::to_string(CUS[p]), done[p] = true;
        printf("%s%s%s\n", head[q].c_str(), cus.c_str(), body[q].c_str());
      }
    }
  return fails ? 1 : 0;
}

} // namespace

int main(int argc, char **argv) {
  if (argc >= 4 && !strcmp(argv[1], "sweep")) return sweep(atoi(argv[2]), atoi(argv[3]) != 0, argc >= 5 && !strcmp(argv[4], "quick"));
  if (argc >= 2 && !strcmp(argv[1], "table")) return table();
  fprintf(stderr, "usage: driver sweep <compute units> <strict 0|1> [quick] | driver table\n");
  return 2;
}
