// Plain structs and constants shared by the MFMA conv's host planner
// (conv_plan.h) and its kernels (conv_mfma.hip). No HIP or torch headers.
#pragma once

#include <cstddef>
#include <type_traits>

namespace ibp {

constexpr int BK = 64;        // K depth per step

struct ConvParams {
  const unsigned short* x;   // NHWC bf16
  const unsigned short* w;   // [Cout][K] bf16 (N-major pack)
  unsigned short* y;         // NHWC bf16 out
  const float* scale;        // optional per-channel scale (folded BN)
  const float* shift;        // optional per-channel shift / bias
  const unsigned short* res;      // optional residual, added BEFORE act
  const unsigned short* res_post; // optional residual, added AFTER act
  const unsigned short* res_post2;
  int N, H, W, Cin, Cout, KH, KW;
  int stride, pad_h, pad_w, dil_h, dil_w, Ho, Wo;
  int zs;                    // gather stride (transposed-conv dgrad), 1 = off
  long long M;               // N*Ho*Wo
  int K;                     // KH*KW*Cin
  int n_mtiles;              // ceil(M/BM)
  int act;                   // leaky-relu on epilogue
  int splitk;                // K-dimension split factor (small-grid layers)
  float* ws;                 // fp32 workspace for split-K partial accumulation
  int vec_epi;               // 1: 4-channel epilogue groups, 2: 8-channel
  int pair_epi;              // fallback may use 2-channel (4-byte) accesses
  int m32;                   // M (+ tile padding) fits 32-bit index math
  // output scatter (nearest-x2 upsample folded into the conv): rows index the
  // LOW-resolution Ho x Wo grid and row (n, i, j) is stored at pixel
  // (n*2Ho + 2i+py)*2Wo + 2j+px of y / res / res_post / res_post2
  int up, py, px;
  // second source of a two-source 1x1 conv (Cin2 = 0: off): K = Cin + Cin2,
  // row m reads x[m*Cin + k] for k < Cin and x2[m*Cin2 + (k - Cin)] past it.
  // The host requires Cin % BK == 0, so a K-chunk never straddles the two.
  int Cin2;
  const unsigned short* x2;  // [M][Cin2] bf16
  // A/B gather of the main loop: 0 = generic (any shape), 1 = tap-uniform
  // (plan_conv sets it; its conditions are listed there)
  int gather;
};

// The tap-uniform gather addresses x and w through range-checked buffer
// loads with UNSIGNED 32-BIT BYTE offsets: both operands must be at most
// kGatherMaxBytes long (plan_conv enforces it), so that every in-range offset
// lies below kGatherOob, the offset the kernel substitutes for a padding tap
// or a row past M / Cout — it is past the end of any such buffer and the
// load returns zeros.
constexpr long long kGatherMaxBytes = 0x7fffffffLL;
constexpr unsigned kGatherOob = 0x80000000u;

// grouped launch: up to kMaxGroup INDEPENDENT convs in one grid
constexpr int kMaxGroup = 8;

struct ConvGroupParams {
  ConvParams p[kMaxGroup];
  int block_end[kMaxGroup];  // exclusive prefix sum of the block counts
  int cfg[kMaxGroup];        // tile_cfg(BM, BN, deep)
  int n;
};

// tile configuration index shared by host and device
constexpr int tile_cfg(int BM, int BN, bool deep) {
  return ((BM == 128 ? (BN == 128 ? 0 : 1) : (BM == 64 ? 2 : 3)) << 1) |
         (deep ? 1 : 0);
}

// the grouped kernel reads its table at offset 0 of the kernel arguments
static_assert(offsetof(ConvGroupParams, p) == 0 &&
                  std::is_standard_layout<ConvGroupParams>::value &&
                  std::is_trivially_copyable<ConvGroupParams>::value &&
                  sizeof(ConvParams) % alignof(ConvParams) == 0 &&
                  sizeof(ConvGroupParams) <= 4096,
              "ConvGroupParams layout: problem array first, within the "
              "kernel-argument limit");

// ConvParams::up as the split-K combine needs it
struct OutScatter {
  int up, py, px, Ho, Wo;
};

struct CombineProblem {
  const float* ws;
  unsigned short* y;
  const float* scale;
  const float* shift;
  const unsigned short* res;
  const unsigned short* res_post;
  const unsigned short* res_post2;
  long long total;
  int C, act, splitk, vec;
  OutScatter os;
};

struct CombineGroupParams {
  CombineProblem c[kMaxGroup];
  int block_end[kMaxGroup];
  int n;
};

}  // namespace ibp
