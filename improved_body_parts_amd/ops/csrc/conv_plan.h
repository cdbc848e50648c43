// Host planner of the MFMA conv: tile, split-K, prefetch depth, epilogue path
// (from pointer alignment), the 32-bit index guards, and for a grouped launch
// the grid order, block prefix sums, workspace sub-allocation and combine
// table. Integer logic over plain structs, no torch, no HIP; pointers are
// compared and offset, never dereferenced (tests/csrc/conv_plan_check.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "conv_params.h"

namespace ibp {

// Tile and split-K choice, from the GEMM extents (and the env overrides).
struct TilePlan {
  int BM, BN, n_mtiles, ntiles, splitk, nk_block;
  bool deep;
};

// One conv to plan. The caller sets what describes it in `p`: the pointers x,
// w, y (allocated by the caller), scale, shift and the residuals; the
// geometry N .. zs (the extension's 15-int row, in its order); act; for one
// output parity of an upfold conv up, py, px. plan_conv derives the rest.
struct ConvProblem {
  ConvParams p{};
  // tile chosen elsewhere (the four parities of an upfold share one)
  std::optional<TilePlan> tile;
};

// Everything decided for one conv: the filled ConvParams (all but the
// workspace pointer, see set_workspace) and the tile. Single and grouped
// launches both run from it: a group member runs what it would run alone.
struct ConvPlan {
  ConvParams p;
  TilePlan t;
  bool vec_combine;    // before the workspace is known: all BUT its alignment
  int nblocks;         // ntiles * splitk
  long long ws_elems;  // fp32 workspace elements (0 when unsplit)
};

inline bool misaligned(const void* ptr, uintptr_t a) {
  return ptr != nullptr && (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) != 0;
}

inline void pick_tile(long long M, int Cout, int& BM, int& BN) {
  // BM: small-M tiles for the hourglass's 8^2/16^2 scales (avoids the 8-16x
  // split-K workspace round-trip measured in round 1); BN: minimise padded
  // cols (Cout=192 as 3x64 beats 2x128 — half the second 128-tile is wasted).
  BM = 128;
  if (M <= 2048) BM = 32;
  else if (M <= 8192) BM = 64;
  if (const char* e = getenv("IBP_CONV_BM")) {
    BM = atoi(e);
    // any other value would run the 32x64 kernel over another tile's n_mtiles
    if (BM != 32 && BM != 64 && BM != 128)
      throw std::invalid_argument(
          std::string("IBP_CONV_BM must be 32, 64 or 128, got '") + e + "'");
  }
  const long long padded128 = ((Cout + 127) / 128) * 128LL;
  const long long padded64 = ((Cout + 63) / 64) * 64LL;
  BN = (BM == 128 && Cout > 64 && padded128 <= padded64) ? 128 : 64;
}

// split-K factor for a grid of `ntiles` output tiles over nk_total K-chunks
inline int pick_split(int ntiles, int nk_total) {
  // split K on small grids so the 256-CU chip stays filled (~2 blocks/CU).
  // Normalise so EVERY slice has work: with raw splitk=7 over nk_total=8 the
  // last 3 slices get no chunks, return early, and the combine kernel then
  // sums their UNINITIALISED workspace slices (silent garbage whenever the
  // allocator hands back dirty memory — found as exploding gradients through
  // the scale-2 Merge convs). tests/test_conv_plan_cpu.py sweeps this.
  int sk_target = 384;
  if (const char* e = getenv("IBP_SPLITK_TARGET")) sk_target = atoi(e);
  int splitk = 1;
  if (ntiles < sk_target && nk_total > 1) {
    splitk = std::min((int)nk_total, (sk_target + ntiles - 1) / ntiles);
    int nk_chunk = ((int)nk_total + splitk - 1) / splitk;
    splitk = ((int)nk_total + nk_chunk - 1) / nk_chunk;
  }
  return splitk;
}

// `parts` problems of M rows each that are one logical conv: the tile is
// picked for parts*M rows and the split for all parts*ntiles tiles; tiles do
// not straddle parts, so n_mtiles and ntiles are per part.
inline TilePlan plan_tiles(long long M, int Cout, int K, int parts) {
  TilePlan t;
  pick_tile(parts * M, Cout, t.BM, t.BN);
  t.n_mtiles = (int)((M + t.BM - 1) / t.BM);
  t.ntiles = t.n_mtiles * ((Cout + t.BN - 1) / t.BN);
  const int nk_total = (K + BK - 1) / BK;
  t.splitk = pick_split(parts * t.ntiles, nk_total);
  // short-K blocks (the 1x1 layers: <= 6 chunks) never reach pipeline
  // steady state with single-stage prefetch — use the 2-deep variant there
  t.nk_block = (nk_total + t.splitk - 1) / t.splitk;
  t.deep = t.nk_block <= 6;
  return t;
}

inline TilePlan plan_tile(long long M, int Cout, int K) {
  return plan_tiles(M, Cout, K, 1);
}

// The four parities of an upfold conv (2x2 taps over M_low low-resolution
// pixels) share one plan. (Planned one by one, the 128^2 refine conv would
// take BM=64 and split 2 although its 1024 tiles already fill the chip.)
inline TilePlan plan_upfold_tile(long long M_low, int Cout, int Cin) {
  return plan_tiles(M_low, Cout, 4 * Cin, 4);
}

// Tap-uniform gather (ConvParams::gather = 1), decided from the finished
// geometry, K, m32 and the x / w pointers. All of:
//   * one source, zs == 1 (no virtual zero-dilated image);
//   * Cin % BK == 0: a K-chunk lies inside one filter tap, so the tap is the
//     same for the whole block, and K % BK == 0: no K-tail;
//   * KH*KW <= 32: a row's in-bounds taps are one 32-bit mask;
//   * x and w 16-byte aligned: with Cin % 64 == 0 every 16-byte piece is;
//   * m32: rows decompose in 32-bit math;
//   * x and w at most kGatherMaxBytes long: the kernel's offsets are unsigned
//     32-bit byte offsets into range-checked buffers (conv_params.h).
// IBP_CONV_GATHER=0 forces the generic gather everywhere (A/B switch).
inline bool gather_eligible(const ConvParams& p) {
  if (const char* e = getenv("IBP_CONV_GATHER"))
    if (e[0] == '0' && e[1] == '\0') return false;
  if (p.x2 != nullptr || p.Cin2 != 0 || p.zs != 1) return false;
  if (p.Cin <= 0 || p.Cin % BK != 0) return false;
  if (p.KH * p.KW < 1 || p.KH * p.KW > 32) return false;
  if (misaligned(p.x, 16) || misaligned(p.w, 16)) return false;
  if (!p.m32) return false;
  const long long x_bytes = 2LL * p.N * p.H * p.W * p.Cin;
  const long long w_bytes = 2LL * p.Cout * p.K;
  return x_bytes <= kGatherMaxBytes && w_bytes <= kGatherMaxBytes;
}

inline ConvPlan plan_conv(const ConvProblem& q) {
  ConvPlan plan;
  plan.p = q.p;
  ConvParams& p = plan.p;
  p.M = (long long)p.N * p.Ho * p.Wo;
  // any Cin is legal: subpieces crossing tap boundaries take the per-element
  // re-derive path (the Cin=3 stem runs there; Cin % 8 == 0 stays vectorized)
  p.K = p.KH * p.KW * p.Cin;
  if (p.x2 != nullptr || p.Cin2 != 0) {
    // two-source 1x1 conv: planned like any conv over K = Cin + Cin2. Source
    // 1 must fill whole K-chunks (the kernel picks the source per chunk) and
    // the gather has no tap walk, so only the plain 1x1 geometry is legal.
    if (p.x2 == nullptr || p.Cin2 <= 0)
      throw std::invalid_argument(
          "two-source conv: x2 and Cin2 > 0 go together");
    if (p.Cin <= 0 || p.Cin % BK != 0)
      throw std::invalid_argument(
          "two-source conv: Cin must be a multiple of 64");
    if (p.KH * p.KW != 1 || p.stride != 1 || p.pad_h != 0 || p.pad_w != 0 ||
        p.dil_h != 1 || p.dil_w != 1 || p.zs != 1 || p.Ho != p.H ||
        p.Wo != p.W)
      throw std::invalid_argument(
          "two-source conv: 1x1, stride 1, unpadded, undilated, zs 1 only");
    if (p.up)
      throw std::invalid_argument(
          "two-source conv: cannot be an upfold parity");
    if (q.tile)
      throw std::invalid_argument(
          "two-source conv: plans its own tile");
    p.K = p.Cin + p.Cin2;
  }
  const TilePlan t = q.tile ? *q.tile : plan_tile(p.M, p.Cout, p.K);
  const int Cout = p.Cout, splitk = t.splitk;
  p.n_mtiles = t.n_mtiles;
  p.splitk = splitk;
  // per-split slices written with plain stores -> an uninitialised workspace
  // is safe (every in-range element is covered by every split's epilogue)
  plan.ws_elems = splitk > 1 ? (long long)splitk * p.M * Cout : 0;
  p.ws = nullptr;
  // vector epilogue: 4-channel groups need Cout % 4 == 0 (then the fp32 slabs
  // are 16-byte aligned at every group) plus 16-byte scale/shift and 8-byte
  // residual and y pointers on the unsplit path.
  // The combine's 8-channel groups need Cout % 8 == 0 and 16 bytes throughout.
  p.vec_epi = Cout % 4 == 0 &&
              (splitk > 1 ||
               !(misaligned(p.scale, 16) || misaligned(p.shift, 16) ||
                 misaligned(p.res, 8) || misaligned(p.res_post, 8) ||
                 misaligned(p.res_post2, 8) || misaligned(p.y, 8)));
  if (p.vec_epi && Cout % 8 == 0 && !misaligned(p.y, 16)) p.vec_epi = 2;
  p.pair_epi = Cout % 2 == 0 &&
               !(misaligned(p.res, 4) || misaligned(p.res_post, 4) ||
                 misaligned(p.res_post2, 4) || misaligned(p.y, 4));
  plan.vec_combine =
      Cout % 8 == 0 &&
      !(misaligned(p.scale, 16) || misaligned(p.shift, 16) ||
        misaligned(p.res, 16) || misaligned(p.res_post, 16) ||
        misaligned(p.res_post2, 16) || misaligned(p.y, 16));
  p.m32 = p.M + t.BM < (1LL << 31);
  // the scatter decomposes rows and output pixels' rows in 32-bit math
  if (p.up && 4 * p.M + 4 * t.BM >= (1LL << 31))
    throw std::invalid_argument(
        "upfold conv: output too large for 32-bit row math");
  p.gather = gather_eligible(p) ? 1 : 0;
  plan.t = t;
  plan.nblocks = t.ntiles * splitk;
  return plan;
}

// the workspace pointer completes a plan (its alignment gates vec_combine)
inline void set_workspace(ConvPlan& plan, float* ws) {
  plan.p.ws = ws;
  plan.vec_combine = plan.vec_combine && !misaligned(ws, 16);
}

// split-K combine grid: 256 threads x one element or 8-channel group, <= 4096
inline int combine_blocks(const ConvPlan& plan) {
  const long long total = plan.p.M * plan.p.Cout;
  const long long work = plan.vec_combine ? total / 8 : total;
  const long long g = (work + 255) / 256;
  return (int)(g < 4096 ? (g > 0 ? g : 1) : 4096);
}

// ---- grouped launch --------------------------------------------------------
// One workspace for all split members of plans[first, last), in list order,
// each slice 16-byte aligned (ws_slice): its size, known before it exists.
inline long long ws_slice(const ConvPlan& plan) {
  return (plan.ws_elems + 3) / 4 * 4;
}
inline long long group_workspace(const std::vector<ConvPlan>& plans,
                                 size_t first, size_t last) {
  long long total = 0;
  for (size_t i = first; i < last; ++i) total += ws_slice(plans[i]);
  return total;
}

struct GroupPlan {
  int order[kMaxGroup];         // grid position -> member (list order)
  long long ws_off[kMaxGroup];  // member -> offset of its workspace slice
  ConvGroupParams g;
  CombineGroupParams cg;        // the split members, in grid order
  int blocks, cblocks;          // grid sizes of the conv and the combine launch
  bool up;                      // all members scatter (upfold) or none does
};

// One grouped conv launch (+ one grouped combine) over plans[first, last),
// at most kMaxGroup of them: points the split members at their slices of the
// workspace at `ws_base` (group_workspace(...) floats) and fills both
// kernel-argument tables. A block writes only its own problem's outputs, so
// grid order never changes a result: most K-chunks first, ties in list order.
inline GroupPlan assemble_group(std::vector<ConvPlan>& plans, size_t first,
                                size_t last, float* ws_base) {
  const int n = (int)(last - first);
  if (n < 1 || n > kMaxGroup || last > plans.size())
    throw std::invalid_argument("grouped conv: 1 to kMaxGroup members");
  GroupPlan gp{};
  gp.up = plans[first].p.up != 0;
  long long ws_total = 0;
  for (int i = 0; i < n; ++i) {
    ConvPlan& plan = plans[first + i];
    if ((plan.p.up != 0) != gp.up)
      throw std::invalid_argument(
          "grouped conv: upfold and plain members cannot mix");
    // the grouped kernels are compiled without the two-source gather
    if (plan.p.Cin2 != 0)
      throw std::invalid_argument(
          "grouped conv: a two-source conv launches on its own");
    gp.order[i] = i;
    gp.ws_off[i] = ws_total;
    if (plan.ws_elems > 0) set_workspace(plan, ws_base + ws_total);
    ws_total += ws_slice(plan);
  }
  std::stable_sort(gp.order, gp.order + n, [&](int a, int b) {
    return plans[first + a].t.nk_block > plans[first + b].t.nk_block;
  });
  // entries past n repeat the last member (the kernels' scans stop at n)
  for (int i = 0; i < kMaxGroup; ++i) {
    const ConvPlan& plan = plans[first + gp.order[i < n ? i : n - 1]];
    if (i < n) gp.blocks += plan.nblocks;
    gp.g.p[i] = plan.p;
    gp.g.cfg[i] = tile_cfg(plan.t.BM, plan.t.BN, plan.t.deep);
    gp.g.block_end[i] = gp.blocks;
  }
  gp.g.n = n;
  int nc = 0;
  for (int i = 0; i < n; ++i) {
    const ConvPlan& plan = plans[first + gp.order[i]];
    if (plan.p.splitk <= 1) continue;
    const ConvParams& p = plan.p;
    gp.cblocks += combine_blocks(plan);
    gp.cg.c[nc] = CombineProblem{p.ws, p.y, p.scale, p.shift, p.res,
                                 p.res_post, p.res_post2,
                                 (long long)p.M * p.Cout, p.Cout, p.act,
                                 p.splitk, plan.vec_combine ? 1 : 0,
                                 OutScatter{p.up, p.py, p.px, p.Ho, p.Wo}};
    gp.cg.block_end[nc++] = gp.cblocks;
  }
  for (int i = nc; i < kMaxGroup; ++i) {
    gp.cg.c[i] = gp.cg.c[nc > 0 ? nc - 1 : 0];
    gp.cg.block_end[i] = gp.cblocks;
  }
  gp.cg.n = nc;
  return gp;
}

}  // namespace ibp
