// MFMA implicit-GEMM convolution for CDNA4 (gfx950), NHWC bf16.
//
// The heart of the framework's compute path: replaces cuDNN/MIOpen convolution
// (the reference delegates ALL conv work to cuDNN) with a
// hand-written bf16 matrix-core kernel:
//
//   C[M = N*Ho*Wo][Cout] = A[M][K = KH*KW*Cin] @ B[K][Cout]
//
//   * A is gathered implicitly from the NHWC input (zero-padding handled by
//     predicated loads); B is the weight pre-packed [Cout][K] row-major.
//   * block tile BMx(BN): (128,128) / (128,64) for big spatial maps,
//     (64,64) / (32,64) for the hourglass's 16^2/8^2 tails (small-M tiles cut
//     split-K workspace traffic 4-8x there — round-1 weak #2).
//   * 4 waves per block arranged (BM/WM)x(BN/WN), each computing WMxWN as
//     AFRAGxBFRAG fragments of v_mfma_f32_16x16x32_bf16, fp32 accumulation.
//   * K loop in BK=64 steps, double-buffered LDS with register staging:
//     tile t+1's global loads are issued before tile t's MFMAs (T14).
//   * LDS rows carry a T2 XOR swizzle — the 16-lane ds_read_b128 group
//     (16 distinct rows, same k-slice) spreads over 8 bank slots.
//   * optional fused epilogue: per-channel scale/shift (folded BatchNorm),
//     PRE-act residual (bottleneck skip), LeakyReLU, then up to two POST-act
//     residuals (hourglass up1+deconv1 join and the cross-stack feature-cache
//     add ride inside the conv kernel on the inference path).
//   * zs (gather stride): reads the virtual zero-dilated image x[hi/zs] when
//     hi % zs == 0 — stride-s dgrad as a stride-1 conv over dilated dy with
//     180-rotated transposed weights.
//   * up (output scatter): a 3x3 conv over a nearest-x2 upsampled map runs as
//     four 2x2 convs over the low-resolution map, one per output parity, with
//     summed weights (pack_upfold_weight_kernel); each parity's rows are
//     stored at its own pixels of the full-resolution output
//     (conv_mfma_upfold_fwd).
//   * two gathers fill the same LDS image. The generic one (below) handles any
//     shape and re-derives addresses, bounds, alignment and K-tail per chunk.
//     The tap-uniform one (TU, ConvParams::gather == 1, chosen by the host
//     planner: one source, zs == 1, Cin % 64 == 0, <= 32 taps, 16-byte
//     aligned x and w, 32-bit rows and byte offsets) computes a row's pixel
//     offset and in-bounds tap mask once per block, walks (kh, kw, ci) in
//     scalar registers, and loads full 128-byte lines (8 lanes x 16 bytes per
//     row) through range-checked buffer loads; padding taps and rows past
//     M / Cout select an out-of-range offset and read zeros. Its main loop
//     has no division, no 64-bit multiply and no branch but its own. Chunk
//     boundaries, fragment layout and MFMA order are shared, so both gathers
//     give the same bits (IBP_CONV_GATHER=0 forces the generic one).
//
// Supported: any KHxKW with Cin % 8 == 0 (per-8 subpieces re-derive their
// filter tap, so Cin 16 s2d-stem tiles and 64..768 hourglass tiles both hit
// the vector path), arbitrary Cin for 1x1 (K-tail predication covers the
// 50-channel merge heads) and via the elementwise tail, stride 1 or 2.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <algorithm>
#include <type_traits>
#include <vector>
#include "common.h"
#include "conv_params.h"   // ConvParams and the launch tables
#include "conv_plan.h"     // the host planner

namespace ibp {

typedef short short8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef unsigned short ushortv8 __attribute__((ext_vector_type(8)));
typedef unsigned short ushortv4 __attribute__((ext_vector_type(4)));

// LDS tile addressing: unpadded BK-short rows with a T2 XOR swizzle — the
// 16-lane ds_read_b128 group (16 distinct rows, same k-slice) spreads over 8
// bank slots (<=2-way) instead of hitting one. k is always a multiple of 8
// here, so the XOR preserves 16-B alignment.
__device__ __forceinline__ int lds_off(int row, int k) {
  return row * BK + (k ^ ((row & 7) << 3));
}

// DEEP: two-stage register prefetch — wins ONLY on short-K shapes (the 1x1
// layers at <= 6 K-chunks never reach pipeline steady state); on long-K 3x3
// shapes the extra register bank measured 10-15% slower.
//
// The body is a device function so that the single-problem kernels and the
// grouped kernel (several independent convs in one launch) share it: `bid`
// is the block id LOCAL to this problem, lds_a/lds_b hold 2*BM*BK and
// 2*BN*BK shorts (double buffer).
//
// UP compiles the output scatter of ConvParams::up in; only the grouped
// upfold kernel instantiates it, every other kernel is the code it was
// without it.
//
// CAT compiles the two-source 1x1 gather of ConvParams::x2 in (and the tap
// walk out); only conv_mfma_kernel<.., true> instantiates it.
template <int BM, int BN, bool DEEP, bool UP, bool CAT, bool TU,
          typename Params>
__device__ __forceinline__ void conv_mfma_body(const Params& p,
                                               const int bid,
                                               unsigned short* lds_a,
                                               unsigned short* lds_b) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  // tile coordinates; with split-K, a tile's K-slices are adjacent block ids
  const int ntiles_n = (p.Cout + BN - 1) / BN;
  const int sk = bid % p.splitk;
  const int tile = bid / p.splitk;
  const int mt = tile / ntiles_n;
  const int nt = tile % ntiles_n;
  const long long m0 = (long long)mt * BM;
  const int n0 = nt * BN;

  // wave sub-tile layout: 4 waves as (BM/WM) x (BN/WN)
  constexpr int WROWS = (BM == 128) ? ((BN == 128) ? 2 : 4) : 2;
  constexpr int WCOLS = 4 / WROWS;
  constexpr int WM = BM / WROWS;
  constexpr int WN = BN / WCOLS;
  constexpr int AFRAG = WM / 16;
  constexpr int BFRAG = WN / 16;
  const int wm = (WCOLS == 1) ? wave : (wave >> 1);
  const int wn = (WCOLS == 1) ? 0 : (wave & 1);
  const int row_base = wm * WM;
  const int col_base = wn * WN;

  floatx4 acc[AFRAG][BFRAG];
  #pragma unroll
  for (int i = 0; i < AFRAG; ++i)
    #pragma unroll
    for (int j = 0; j < BFRAG; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  // ---- staging geometry: 256 threads cover BM*BK (A) and BN*BK (B) shorts
  constexpr int A_ELEMS = BM * BK / 256;   // 32 / 16 / 8
  constexpr int B_ELEMS = BN * BK / 256;   // 32 / 16
  constexpr int TPR_A = BK / A_ELEMS;
  constexpr int TPR_B = BK / B_ELEMS;
  const int a_row = tid / TPR_A;
  const int a_off = (tid % TPR_A) * A_ELEMS;
  const int b_row = tid / TPR_B;
  const int b_off = (tid % TPR_B) * B_ELEMS;

  // per-row output-pixel decomposition for the A gather
  const long long a_m = m0 + a_row;
  int a_n = 0, a_ho = 0, a_wo = 0;
  bool a_valid_row = a_m < p.M;
  if (a_valid_row && p.m32) {
    // 64-bit % and / are emulated (dozens of instructions each); these
    // blocks live for a few microseconds, so the common case stays 32-bit
    unsigned t = (unsigned)a_m;
    a_wo = (int)(t % (unsigned)p.Wo); t /= (unsigned)p.Wo;
    a_ho = (int)(t % (unsigned)p.Ho);
    a_n = (int)(t / (unsigned)p.Ho);
  } else if (a_valid_row) {
    long long t = a_m;
    a_wo = (int)(t % p.Wo); t /= p.Wo;
    a_ho = (int)(t % p.Ho);
    a_n = (int)(t / p.Ho);
  }
  const int hi_base = a_ho * p.stride - p.pad_h;
  const int wi_base = a_wo * p.stride - p.pad_w;

  const int nk_total = (p.K + BK - 1) / BK;
  const int nk_chunk = (nk_total + p.splitk - 1) / p.splitk;
  const int k_begin = sk * nk_chunk;
  const int nk = min(nk_chunk, nk_total - k_begin);
  if (nk <= 0) return;

  unsigned short a_reg0[A_ELEMS];
  unsigned short b_reg0[B_ELEMS];
  // second bank referenced only under `if constexpr (DEEP)` — fully
  // eliminated in the default instantiations
  unsigned short a_reg1[A_ELEMS];
  unsigned short b_reg1[B_ELEMS];

  // ---- incremental tap-walking state for the A gather ----------------------
  // k = (kh*KW + kw)*Cin + ci decodes with ONE division pair at setup; each
  // chunk then advances (ci, kh, kw) by small wrap steps. The first version
  // of the per-8 gather re-divided per subpiece (4 integer divisions per
  // chunk per thread) and measured 0.63-0.68x of the round-1 kernel — the
  // emulated 32-bit divide beside MFMAs is exactly the anti-lever the guide
  // warns about.
  // (CAT: a 1x1 conv over two sources has no taps; k alone is walked)
  int t_kk = k_begin * BK + a_off;
  int t_ci = 0, t_kh = 0, t_kw = 0;
  if constexpr (!CAT) {
    const int t_f = t_kk / p.Cin;
    t_ci = t_kk - t_f * p.Cin;
    t_kh = t_f / p.KW;
    t_kw = t_f - t_kh * p.KW;
  }
  auto tap_advance = [&](int& ci, int& kh, int& kw, int step) {
    ci += step;
    while (ci >= p.Cin) {
      ci -= p.Cin;
      if (++kw == p.KW) { kw = 0; ++kh; }
    }
  };

  // ---- stage the NEXT sequential chunk into registers ----------------------
  // (must be called with consecutive chunks — the tap state walks forward)
  auto load_chunk = [&](int ck, unsigned short (&a_reg)[A_ELEMS],
                        unsigned short (&b_reg)[B_ELEMS]) {
    int kk = t_kk, ci = t_ci, kh = t_kh, kw = t_kw;
    if constexpr (CAT) {
      // two sources, one row index: the chunk lies in x (k < Cin) or in x2 —
      // Cin % BK == 0, so the choice is uniform over the block. x2's width
      // may be anything: pieces past its end are zero (K-tail), rows that
      // are not 16-byte aligned (the 50-channel pred) load per element.
      const bool second = t_kk >= p.Cin;
      const int C = second ? p.Cin2 : p.Cin;
      const int c0 = second ? t_kk - p.Cin : t_kk;
      const unsigned short* src =
          (second ? p.x2 : p.x) + (long long)a_m * C + c0;
      const bool aligned = ((reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
      if (a_valid_row && aligned && c0 + A_ELEMS <= C) {
        #pragma unroll
        for (int v = 0; v < A_ELEMS / 8; ++v)
          *reinterpret_cast<ushortv8*>(&a_reg[v * 8]) =
              *reinterpret_cast<const ushortv8*>(src + v * 8);
      } else {
        #pragma unroll
        for (int e = 0; e < A_ELEMS; ++e)
          a_reg[e] = (a_valid_row && c0 + e < C) ? src[e] : (unsigned short)0;
      }
      goto a_done;
    }
    // fast path: the whole A_ELEMS piece inside one filter tap (all the
    // Cin % 64 == 0 hourglass convs) — ONE predicate set, straight-line
    // vector loads (the per-subpiece form below costs ~10% on hot shapes)
    if (ci + A_ELEMS <= p.Cin && kk + A_ELEMS <= p.K && p.zs == 1) {
      const int hi = hi_base + kh * p.dil_h;
      const int wi = wi_base + kw * p.dil_w;
      const bool ok = a_valid_row && hi >= 0 && hi < p.H &&
                      wi >= 0 && wi < p.W;
      const unsigned short* src =
          p.x + (((long long)a_n * p.H + hi) * p.W + wi) * p.Cin + ci;
      const bool aligned = ((reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
      if (ok && aligned) {
        #pragma unroll
        for (int v = 0; v < A_ELEMS / 8; ++v)
          *reinterpret_cast<ushortv8*>(&a_reg[v * 8]) =
              *reinterpret_cast<const ushortv8*>(src + v * 8);
      } else if (ok) {
        #pragma unroll
        for (int e = 0; e < A_ELEMS; ++e) a_reg[e] = src[e];
      } else {
        #pragma unroll
        for (int e = 0; e < A_ELEMS; ++e) a_reg[e] = 0;
      }
      goto a_done;
    }
    #pragma unroll
    for (int v8 = 0; v8 < A_ELEMS / 8; ++v8) {
      unsigned short* dst = &a_reg[v8 * 8];
      int hi = hi_base + kh * p.dil_h;
      int wi = wi_base + kw * p.dil_w;
      bool ok = a_valid_row;
      if (p.zs > 1) {                    // virtual zero-dilated image (dgrad)
        ok = ok && (hi % p.zs == 0) && (wi % p.zs == 0);
        hi /= p.zs; wi /= p.zs;
      }
      ok = ok && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
      const unsigned short* src =
          p.x + (((long long)a_n * p.H + hi) * p.W + wi) * p.Cin + ci;
      // 16-B vector loads need a 16-B-aligned source (odd Cin, e.g. the
      // 50-channel merge input, makes pixel rows only 2-B aligned)
      const bool aligned = ((reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
      const bool in_tap = ci + 8 <= p.Cin;
      if (ok && aligned && in_tap && kk + 8 <= p.K) {
        *reinterpret_cast<ushortv8*>(dst) =
            *reinterpret_cast<const ushortv8*>(src);
      } else if (ok && in_tap) {
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          // K-tail (1x1 heads): elements past K are zero
          dst[e] = (kk + e < p.K) ? src[e] : (unsigned short)0;
        }
      } else if (!in_tap && a_valid_row) {
        // subpiece crosses tap boundaries (Cin=3 stem, Cin % 8 != 0):
        // walk tap/coordinates element by element (no divisions)
        int cie = ci, khe = kh, kwe = kw;
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          unsigned short v = 0;
          if (kk + e < p.K) {
            int hie = hi_base + khe * p.dil_h;
            int wie = wi_base + kwe * p.dil_w;
            bool oke = true;
            if (p.zs > 1) {
              oke = (hie % p.zs == 0) && (wie % p.zs == 0);
              hie /= p.zs; wie /= p.zs;
            }
            if (oke && hie >= 0 && hie < p.H && wie >= 0 && wie < p.W)
              v = p.x[(((long long)a_n * p.H + hie) * p.W + wie) * p.Cin + cie];
          }
          dst[e] = v;
          if (++cie == p.Cin) {
            cie = 0;
            if (++kwe == p.KW) { kwe = 0; ++khe; }
          }
        }
      } else {
        #pragma unroll
        for (int e = 0; e < 8; ++e) dst[e] = 0;
      }
      kk += 8;
      tap_advance(ci, kh, kw, 8);
    }
a_done:
    // walk the persistent state one full chunk forward
    t_kk += BK;
    if constexpr (!CAT) tap_advance(t_ci, t_kh, t_kw, BK);
    // ---- B: packed [Cout][K] rows
    {
      int col = n0 + b_row;
      int kk = ck * BK + b_off;
      bool ok = col < p.Cout;
      const unsigned short* src = p.w + (long long)col * p.K + kk;
      bool b_aligned = ((reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
      if (ok && b_aligned && kk + B_ELEMS <= p.K) {
        #pragma unroll
        for (int v = 0; v < B_ELEMS / 8; ++v)
          *reinterpret_cast<ushortv8*>(&b_reg[v * 8]) =
              *reinterpret_cast<const ushortv8*>(src + v * 8);
      } else {
        #pragma unroll
        for (int e = 0; e < B_ELEMS; ++e)
          b_reg[e] = (ok && kk + e < p.K) ? src[e] : 0;
      }
    }
  };

  // ---- tap-uniform gather (TU; ConvParams::gather == 1) ---------------------
  // The planner guarantees Cin % BK == 0 (a K-chunk lies inside ONE filter tap,
  // the same for the whole block), no K-tail, zs == 1, m32, 16-byte aligned x
  // and w, and both operands addressable with unsigned 32-bit byte offsets.
  // Staging map: a 16-byte piece per lane, eight consecutive lanes cover one
  // row's 128 bytes of the chunk (full lines), a thread's pieces lie 32 rows
  // apart. The LDS image is the generic one.
  //   per row, once:   byte offset of pixel (n, ho*stride - pad_h,
  //                    wo*stride - pad_w) plus the lane's piece (may be
  //                    "negative": unsigned wrap-around, exact once an
  //                    in-bounds tap is added), and a bit per tap that is in
  //                    bounds for the row (0 for rows past M)
  //   per block:       (kh, kw, ci) in scalar registers, walked by BK
  //   per chunk/piece: one add, one bit test, one select, the 16-byte load
  // Padding taps and rows past M / Cout select the offset kGatherOob, which
  // the buffer's range check answers with zeros: no branch, no zero fill.
  constexpr int A_PIECES = A_ELEMS / 8;
  constexpr int B_PIECES = B_ELEMS / 8;
  typedef unsigned int uintv4 __attribute__((ext_vector_type(4)));
  const int g_row = tid >> 3;          // rows g_row + 32 * j
  const int g_k = (tid & 7) * 8;       // the lane's piece of the chunk
  unsigned tu_abase[TU ? A_PIECES : 1];
  unsigned tu_amask[TU ? A_PIECES : 1];
  unsigned tu_boff[TU ? B_PIECES : 1];
  int tu_ci = 0, tu_kh = 0, tu_kw = 0;  // block-uniform tap of the next chunk
  unsigned tu_bk = 0;                   // byte offset of that chunk in a w row
  unsigned tu_dh = 0, tu_dw = 0;        // bytes per kh / kw step
  // range-checked views of x and w, exactly as long as the operands (the
  // type has no empty value; without TU nothing uses them and they compile
  // away)
  const unsigned pix = (unsigned)p.Cin * 2u;   // bytes per pixel
  const __amdgpu_buffer_rsrc_t tu_xbuf = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(p.x), 0,
      (int)((unsigned)p.N * (unsigned)p.H * (unsigned)p.W * pix), 0x00020000);
  const __amdgpu_buffer_rsrc_t tu_wbuf = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(p.w), 0,
      (int)((unsigned)p.Cout * (unsigned)p.K * 2u), 0x00020000);
  if constexpr (TU) {
    tu_dh = (unsigned)(p.dil_h * p.W) * pix;
    tu_dw = (unsigned)p.dil_w * pix;
    const int kk0 = k_begin * BK;
    const int f0 = kk0 / p.Cin;
    tu_ci = kk0 - f0 * p.Cin;
    tu_kh = f0 / p.KW;
    tu_kw = f0 - tu_kh * p.KW;
    tu_bk = (unsigned)kk0 * 2u;
    // the first row is decomposed once, the others carry-walk from it
    unsigned t = (unsigned)m0 + (unsigned)g_row;
    int wo = (int)(t % (unsigned)p.Wo); t /= (unsigned)p.Wo;
    int ho = (int)(t % (unsigned)p.Ho);
    int n = (int)(t / (unsigned)p.Ho);
    #pragma unroll
    for (int j = 0; j < A_PIECES; ++j) {
      const int hb = ho * p.stride - p.pad_h;
      const int wb = wo * p.stride - p.pad_w;
      unsigned colm = 0, mask = 0;
      for (int kw = 0; kw < p.KW; ++kw)
        if ((unsigned)(wb + kw * p.dil_w) < (unsigned)p.W) colm |= 1u << kw;
      for (int kh = 0; kh < p.KH; ++kh)
        if ((unsigned)(hb + kh * p.dil_h) < (unsigned)p.H)
          mask |= colm << (kh * p.KW);
      tu_amask[j] = (m0 + g_row + 32 * j < p.M) ? mask : 0u;
      tu_abase[j] =
          (((unsigned)n * (unsigned)p.H + (unsigned)hb) * (unsigned)p.W +
           (unsigned)wb) * pix + (unsigned)g_k * 2u;
      wo += 32;
      while (wo >= p.Wo) {
        wo -= p.Wo;
        if (++ho == p.Ho) { ho = 0; ++n; }
      }
    }
    #pragma unroll
    for (int j = 0; j < B_PIECES; ++j) {
      const int col = n0 + g_row + 32 * j;
      tu_boff[j] = col < p.Cout
          ? (unsigned)col * (unsigned)p.K * 2u + (unsigned)g_k * 2u
          : kGatherOob;
    }
  }
  // stage the NEXT sequential chunk (TU): the tap state walks forward
  auto load_chunk_tu = [&](unsigned short (&a_reg)[A_ELEMS],
                           unsigned short (&b_reg)[B_ELEMS]) {
    const unsigned tap = (unsigned)tu_kh * tu_dh + (unsigned)tu_kw * tu_dw +
                         (unsigned)tu_ci * 2u;
    const unsigned bit = 1u << (tu_kh * p.KW + tu_kw);
    #pragma unroll
    for (int j = 0; j < A_PIECES; ++j) {
      const unsigned off =
          (tu_amask[j] & bit) ? tu_abase[j] + tap : kGatherOob;
      *reinterpret_cast<uintv4*>(&a_reg[j * 8]) =
          __builtin_amdgcn_raw_buffer_load_b128(tu_xbuf, (int)off, 0, 0);
    }
    #pragma unroll
    for (int j = 0; j < B_PIECES; ++j)
      *reinterpret_cast<uintv4*>(&b_reg[j * 8]) =
          __builtin_amdgcn_raw_buffer_load_b128(tu_wbuf, (int)tu_boff[j],
                                                (int)tu_bk, 0);
    // scalar walk to the next chunk (selects, no branch)
    tu_bk += BK * 2u;
    tu_ci += BK;
    const bool tap_end = tu_ci >= p.Cin;
    tu_ci = tap_end ? 0 : tu_ci;
    tu_kw += tap_end ? 1 : 0;
    const bool row_end = tu_kw >= p.KW;
    tu_kw = row_end ? 0 : tu_kw;
    tu_kh += row_end ? 1 : 0;
  };
  auto write_chunk_tu = [&](int buf, unsigned short (&a_reg)[A_ELEMS],
                            unsigned short (&b_reg)[B_ELEMS]) {
    #pragma unroll
    for (int j = 0; j < A_PIECES; ++j)
      *reinterpret_cast<ushortv8*>(
          &lds_a[buf * (BM * BK) + lds_off(g_row + 32 * j, g_k)]) =
          *reinterpret_cast<const ushortv8*>(&a_reg[j * 8]);
    #pragma unroll
    for (int j = 0; j < B_PIECES; ++j)
      *reinterpret_cast<ushortv8*>(
          &lds_b[buf * (BN * BK) + lds_off(g_row + 32 * j, g_k)]) =
          *reinterpret_cast<const ushortv8*>(&b_reg[j * 8]);
  };

  auto write_chunk = [&](int buf, unsigned short (&a_reg)[A_ELEMS],
                         unsigned short (&b_reg)[B_ELEMS]) {
    #pragma unroll
    for (int v = 0; v < A_ELEMS / 8; ++v)
      *reinterpret_cast<ushortv8*>(&lds_a[buf * (BM * BK) + lds_off(a_row, a_off + v * 8)]) =
          *reinterpret_cast<const ushortv8*>(&a_reg[v * 8]);
    #pragma unroll
    for (int v = 0; v < B_ELEMS / 8; ++v)
      *reinterpret_cast<ushortv8*>(&lds_b[buf * (BN * BK) + lds_off(b_row, b_off + v * 8)]) =
          *reinterpret_cast<const ushortv8*>(&b_reg[v * 8]);
  };

  // ---- MFMA over one LDS buffer --------------------------------------------
  auto compute = [&](int buf) {
    const int l15 = lane & 15;
    const int kslice = (lane >> 4) * 8;
    #pragma unroll
    for (int kk = 0; kk < BK; kk += 32) {
      short8 afrag[AFRAG], bfrag[BFRAG];
      #pragma unroll
      for (int i = 0; i < AFRAG; ++i)
        afrag[i] = *reinterpret_cast<const short8*>(
            &lds_a[buf * (BM * BK) + lds_off(row_base + i * 16 + l15, kk + kslice)]);
      #pragma unroll
      for (int j = 0; j < BFRAG; ++j)
        bfrag[j] = *reinterpret_cast<const short8*>(
            &lds_b[buf * (BN * BK) + lds_off(col_base + j * 16 + l15, kk + kslice)]);
      // weight fragment FIRST: D[row][col] is then (channel, pixel), which
      // gives each lane 4 consecutive channels of one pixel (see epilogue)
      #pragma unroll
      for (int i = 0; i < AFRAG; ++i)
        #pragma unroll
        for (int j = 0; j < BFRAG; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              bfrag[j], afrag[i], acc[i][j], 0, 0, 0);
    }
  };

  // ---- main loop: register-staged double buffer ----------------------------
  if constexpr (TU && DEEP) {
    // the DEEP schedule below with the tap-uniform gather
    load_chunk_tu(a_reg0, b_reg0);
    write_chunk_tu(0, a_reg0, b_reg0);
    if (nk > 1) load_chunk_tu(a_reg1, b_reg1);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      if (t + 2 < nk) load_chunk_tu(a_reg0, b_reg0);
      compute(0);
      if (t + 1 < nk) write_chunk_tu(1, a_reg1, b_reg1);
      __syncthreads();
      if (++t >= nk) break;
      if (t + 2 < nk) load_chunk_tu(a_reg1, b_reg1);
      compute(1);
      if (t + 1 < nk) write_chunk_tu(0, a_reg0, b_reg0);
      __syncthreads();
    }
  } else if constexpr (TU) {
    // the single-stage schedule below with its last step peeled off, so the
    // loop body holds no test of its own: load t+1, MFMA t, write t+1, barrier
    load_chunk_tu(a_reg0, b_reg0);
    write_chunk_tu(0, a_reg0, b_reg0);
    __syncthreads();
    for (int t = 0; t + 1 < nk; ++t) {
      load_chunk_tu(a_reg0, b_reg0);
      compute(t & 1);
      write_chunk_tu((t + 1) & 1, a_reg0, b_reg0);
      __syncthreads();
    }
    compute((nk - 1) & 1);
  } else if constexpr (DEEP) {
    // 2-deep prefetch: chunk t+2's loads issue at iteration t, land at t+1
    load_chunk(k_begin, a_reg0, b_reg0);
    write_chunk(0, a_reg0, b_reg0);
    if (nk > 1) load_chunk(k_begin + 1, a_reg1, b_reg1);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      if (t + 2 < nk) load_chunk(k_begin + t + 2, a_reg0, b_reg0);
      compute(0);
      if (t + 1 < nk) write_chunk(1, a_reg1, b_reg1);
      __syncthreads();
      if (++t >= nk) break;
      if (t + 2 < nk) load_chunk(k_begin + t + 2, a_reg1, b_reg1);
      compute(1);
      if (t + 1 < nk) write_chunk(0, a_reg0, b_reg0);
      __syncthreads();
    }
  } else {
    load_chunk(k_begin, a_reg0, b_reg0);
    write_chunk(0, a_reg0, b_reg0);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      if (t + 1 < nk) load_chunk(k_begin + t + 1, a_reg0, b_reg0);
      compute(t & 1);
      // writing buf[(t+1)&1] is safe without a barrier: its last readers
      // were separated by the end-of-iteration barrier of step t-1
      if (t + 1 < nk) write_chunk((t + 1) & 1, a_reg0, b_reg0);
      __syncthreads();
    }
  }

  // ---- epilogue ------------------------------------------------------------
  // compute() feeds the weight fragment as the first MFMA operand, so the C/D
  // lane map (row = (lane>>4)*4 + r, col = lane&15) reads (channel, pixel):
  // a lane's 4 accumulators are 4 CONSECUTIVE CHANNELS of one pixel. Paths,
  // widest first (the host picks by Cout and pointer alignment):
  //   vec_epi 2  Cout % 8 == 0, unsplit: 16-byte bf16 stores (lane exchange)
  //   vec_epi 1+ Cout % 4 == 0: 8-byte bf16 stores / 16-byte fp32 slab stores
  //   pair_epi   Cout % 2 == 0: 4-byte bf16 stores / 8-byte slab stores
  //   otherwise  per element
  // All four do the same arithmetic in the same order.
  const int epix = lane & 15;
  const int ech4 = (lane >> 4) * 4;
  float* const ws_slice =
      p.splitk > 1 ? p.ws + (long long)sk * p.M * p.Cout : nullptr;
  // UP: output pixel of each of this lane's AFRAG rows (16 apart) — the
  // first row is decomposed once in 32-bit math (the host only sets `up`
  // with m32), the rest carry-walk; the fp32 slabs stay in row order, their
  // combine does the same scatter.
  long long opix[UP ? AFRAG : 1];
  if constexpr (UP) {
    unsigned t = (unsigned)(m0 + row_base + epix);
    int oj = (int)(t % (unsigned)p.Wo); t /= (unsigned)p.Wo;
    int oi = (int)(t % (unsigned)p.Ho);
    int on = (int)(t / (unsigned)p.Ho);
    #pragma unroll
    for (int i = 0; i < AFRAG; ++i) {
      opix[i] = ((long long)on * (2 * p.Ho) + 2 * oi + p.py) * (2 * p.Wo) +
                2 * oj + p.px;
      oj += 16;
      while (oj >= p.Wo) {
        oj -= p.Wo;
        if (++oi == p.Ho) { oi = 0; ++on; }
      }
    }
  }
  // element index in y / residuals of (row slot i, channel c), given the
  // row-order index `lin` = m * Cout + c that the slabs use
  auto out_idx = [&](int i, int c, long long lin) -> long long {
    if constexpr (UP) return opix[i] * p.Cout + c;
    else return lin;
  };
  // fused epilogue of one fragment: 8-byte residual loads, today's order
  auto finish = [&](const floatx4& a, long long idx, const floatx4& sc,
                    const floatx4& sh) -> ushortv4 {
    ushortv4 r0 = ushortv4{0, 0, 0, 0}, r1 = r0, r2 = r0;
    if (p.res) r0 = *reinterpret_cast<const ushortv4*>(p.res + idx);
    if (p.res_post) r1 = *reinterpret_cast<const ushortv4*>(p.res_post + idx);
    if (p.res_post2)
      r2 = *reinterpret_cast<const ushortv4*>(p.res_post2 + idx);
    ushortv4 out;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = a[r] * sc[r] + sh[r];
      if (p.res) v += us2f(r0[r]);
      if (p.act) v = leaky(v, 0.01f);
      if (p.res_post) v += us2f(r1[r]);
      if (p.res_post2) v += us2f(r2[r]);
      out[r] = f2us(v);
    }
    return out;
  };
  if (p.vec_epi == 2 && p.splitk == 1) {
    // Cout % 8 == 0: lanes l and l^16 (same pixel, adjacent channel groups)
    // trade one finished fragment each, so every lane owns 8 consecutive
    // channels and stores 16 bytes. Both lanes of a pair take the same
    // branches (same pixel; an 8-channel group is in range as a whole).
    const bool odd = (lane >> 4) & 1;
    #pragma unroll
    for (int jp = 0; jp < BFRAG; jp += 2) {
      const int col0 = n0 + col_base + jp * 16 + ech4;
      const int col1 = col0 + 16;
      if (col0 >= p.Cout) continue;
      const bool ok1 = col1 < p.Cout;
      floatx4 sc0 = floatx4{1.f, 1.f, 1.f, 1.f}, sc1 = sc0;
      floatx4 sh0 = floatx4{0.f, 0.f, 0.f, 0.f}, sh1 = sh0;
      if (p.scale) sc0 = *reinterpret_cast<const floatx4*>(p.scale + col0);
      if (p.shift) sh0 = *reinterpret_cast<const floatx4*>(p.shift + col0);
      if (p.scale && ok1)
        sc1 = *reinterpret_cast<const floatx4*>(p.scale + col1);
      if (p.shift && ok1)
        sh1 = *reinterpret_cast<const floatx4*>(p.shift + col1);
      #pragma unroll
      for (int i = 0; i < AFRAG; ++i) {
        const long long m = m0 + row_base + i * 16 + epix;
        if (m >= p.M) continue;
        const long long idx0 = out_idx(i, col0, m * p.Cout + col0);
        union { ushortv4 v; unsigned u[2]; } o0, o1, rx;
        o0.v = finish(acc[i][jp], idx0, sc0, sh0);
        o1.v = ushortv4{0, 0, 0, 0};
        if (ok1) o1.v = finish(acc[i][jp + 1], idx0 + 16, sc1, sh1);
        rx.u[0] = __shfl_xor(odd ? o0.u[0] : o1.u[0], 16, 64);
        rx.u[1] = __shfl_xor(odd ? o0.u[1] : o1.u[1], 16, 64);
        union { ushortv8 v; unsigned u[4]; } st;
        if (!odd) {          // channels col0 .. col0+7
          st.u[0] = o0.u[0]; st.u[1] = o0.u[1];
          st.u[2] = rx.u[0]; st.u[3] = rx.u[1];
          *reinterpret_cast<ushortv8*>(p.y + idx0) = st.v;
        } else if (ok1) {    // channels col1-4 .. col1+3
          st.u[0] = rx.u[0]; st.u[1] = rx.u[1];
          st.u[2] = o1.u[0]; st.u[3] = o1.u[1];
          *reinterpret_cast<ushortv8*>(p.y + idx0 + 12) = st.v;
        }
      }
    }
    return;
  }
  #pragma unroll
  for (int j = 0; j < BFRAG; ++j) {
    const int col = n0 + col_base + j * 16 + ech4;
    if (col >= p.Cout) continue;
    if (p.vec_epi) {
      // Cout % 4 == 0 and col % 4 == 0: the whole group is in range, and
      // every pointer touched below is aligned for its access (host check)
      floatx4 sc = floatx4{1.f, 1.f, 1.f, 1.f};
      floatx4 sh = floatx4{0.f, 0.f, 0.f, 0.f};
      if (p.splitk == 1) {
        if (p.scale) sc = *reinterpret_cast<const floatx4*>(p.scale + col);
        if (p.shift) sh = *reinterpret_cast<const floatx4*>(p.shift + col);
      }
      #pragma unroll
      for (int i = 0; i < AFRAG; ++i) {
        const long long m = m0 + row_base + i * 16 + epix;
        if (m >= p.M) continue;
        const long long lin = m * p.Cout + col;
        if (p.splitk > 1) {
          // each K-split owns a workspace slice: plain stores, no zero-init,
          // no atomics, deterministic sums (combine kernel reduces slices)
          *reinterpret_cast<floatx4*>(ws_slice + lin) = acc[i][j];
          continue;
        }
        const long long idx = out_idx(i, col, lin);
        *reinterpret_cast<ushortv4*>(p.y + idx) =
            finish(acc[i][j], idx, sc, sh);
      }
      continue;
    }
    if (p.pair_epi) {
      // even Cout (the 50-channel heads): 2-channel groups, 4-byte accesses;
      // col + r is even, so a pair never straddles Cout
      #pragma unroll
      for (int r = 0; r < 4; r += 2) {
        if (col + r >= p.Cout) continue;
        const float sc0 = p.scale ? p.scale[col + r] : 1.f;
        const float sc1 = p.scale ? p.scale[col + r + 1] : 1.f;
        const float sh0 = p.shift ? p.shift[col + r] : 0.f;
        const float sh1 = p.shift ? p.shift[col + r + 1] : 0.f;
        #pragma unroll
        for (int i = 0; i < AFRAG; ++i) {
          const long long m = m0 + row_base + i * 16 + epix;
          if (m >= p.M) continue;
          const long long lin = m * p.Cout + col + r;
          if (p.splitk > 1) {
            *reinterpret_cast<floatx2*>(ws_slice + lin) =
                floatx2{acc[i][j][r], acc[i][j][r + 1]};
            continue;
          }
          const long long idx = out_idx(i, col + r, lin);
          unsigned r0 = 0, r1 = 0, r2 = 0;
          if (p.res) r0 = *reinterpret_cast<const unsigned*>(p.res + idx);
          if (p.res_post)
            r1 = *reinterpret_cast<const unsigned*>(p.res_post + idx);
          if (p.res_post2)
            r2 = *reinterpret_cast<const unsigned*>(p.res_post2 + idx);
          float v0 = acc[i][j][r] * sc0 + sh0;
          float v1 = acc[i][j][r + 1] * sc1 + sh1;
          if (p.res) {
            v0 += us2f((unsigned short)r0); v1 += us2f((unsigned short)(r0 >> 16));
          }
          if (p.act) { v0 = leaky(v0, 0.01f); v1 = leaky(v1, 0.01f); }
          if (p.res_post) {
            v0 += us2f((unsigned short)r1); v1 += us2f((unsigned short)(r1 >> 16));
          }
          if (p.res_post2) {
            v0 += us2f((unsigned short)r2); v1 += us2f((unsigned short)(r2 >> 16));
          }
          *reinterpret_cast<unsigned*>(p.y + idx) =
              (unsigned)f2us(v0) | ((unsigned)f2us(v1) << 16);
        }
      }
      continue;
    }
    // per-element path: odd Cout or an under-aligned operand
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (col + r >= p.Cout) continue;
      const float sc = p.scale ? p.scale[col + r] : 1.f;
      const float sh = p.shift ? p.shift[col + r] : 0.f;
      #pragma unroll
      for (int i = 0; i < AFRAG; ++i) {
        const long long m = m0 + row_base + i * 16 + epix;
        if (m >= p.M) continue;
        const long long lin = m * p.Cout + col + r;
        if (p.splitk > 1) {
          ws_slice[lin] = acc[i][j][r];
          continue;
        }
        const long long idx = out_idx(i, col + r, lin);
        float v = acc[i][j][r] * sc + sh;
        if (p.res) v += us2f(p.res[idx]);
        if (p.act) v = leaky(v, 0.01f);
        if (p.res_post) v += us2f(p.res_post[idx]);
        if (p.res_post2) v += us2f(p.res_post2[idx]);
        p.y[idx] = f2us(v);
      }
    }
  }
}

// TU compiles the tap-uniform gather in instead of the generic one; the host
// launches it for plans with ConvParams::gather == 1 (never with CAT).
template <int BM, int BN, bool DEEP = false, bool CAT = false, bool TU = false>
__global__ __launch_bounds__(256, 2) void conv_mfma_kernel(ConvParams p) {
  static_assert(!(CAT && TU), "the two-source conv keeps its own gather");
  __shared__ unsigned short lds_a[2 * BM * BK];
  __shared__ unsigned short lds_b[2 * BN * BK];
  conv_mfma_body<BM, BN, DEEP, false, CAT, TU>(p, blockIdx.x, lds_a, lds_b);
}

// ---- grouped launch --------------------------------------------------------
// Up to kMaxGroup INDEPENDENT convs in one grid. The problem table rides the
// kernel arguments; block_end[i] is the exclusive prefix sum of the problems'
// block counts, so a block finds its problem with a scan of at most
// kMaxGroup - 1 uniform compares, then runs the <BM,BN,DEEP> body that the
// problem would get alone, with a problem-local block id. Every block writes
// only its own problem's outputs, so the order of problems in the grid never
// changes a result; the host puts the blocks with the most K-chunks first.
//
// <true> is the upfold launch: every problem is one output parity of a
// nearest-x2-upsample-folded conv and scatters its rows (ConvParams::up).
template <bool UP>
__global__ __launch_bounds__(256, 2) void conv_mfma_grouped_kernel(
    ConvGroupParams g) {
  // one static buffer sized for the largest tile (128x128: 2 x 32 KB); the
  // smaller configurations carve their lds_a / lds_b out of its front
  __shared__ __attribute__((aligned(16))) unsigned short lds[4 * 128 * BK];
  const int gb = blockIdx.x;
  int pi = 0, base = 0, cfg = g.cfg[0];
  #pragma unroll
  for (int i = 0; i < kMaxGroup - 1; ++i) {
    if (i + 1 < g.n && gb >= g.block_end[i]) {
      pi = i + 1;
      base = g.block_end[i];
      cfg = g.cfg[i + 1];
    }
  }
  // A dynamic index into a by-value kernel argument makes the compiler keep
  // a private copy of the whole table (1.5 KB of scratch per lane). Read the
  // chosen entry straight from the kernel-argument segment instead — `g` is
  // the only argument, so it starts at offset 0 — which stays scalar loads
  // with a uniform offset.
  typedef __attribute__((address_space(4))) const char* kernarg_bytes;
  kernarg_bytes ka = (kernarg_bytes)__builtin_amdgcn_kernarg_segment_ptr();
  typedef __attribute__((address_space(4))) const ConvParams* kernarg_params;
  const auto& p = *(kernarg_params)(ka + offsetof(ConvGroupParams, p) +
                                    (size_t)pi * sizeof(ConvParams));
  const int bid = gb - base;
  // the member's gather (ConvParams::gather) rides above the cfg bits
  #define IBP_BODY(BM_, BN_, DEEP_, TU_)                                     \
    conv_mfma_body<BM_, BN_, DEEP_, UP, false, TU_>(p, bid, lds,            \
                                                    lds + 2 * BM_ * BK)
  switch (cfg | (p.gather ? 8 : 0)) {
    case tile_cfg(128, 128, false): IBP_BODY(128, 128, false, false); break;
    case tile_cfg(128, 128, true): IBP_BODY(128, 128, true, false); break;
    case tile_cfg(128, 64, false): IBP_BODY(128, 64, false, false); break;
    case tile_cfg(128, 64, true): IBP_BODY(128, 64, true, false); break;
    case tile_cfg(64, 64, false): IBP_BODY(64, 64, false, false); break;
    case tile_cfg(64, 64, true): IBP_BODY(64, 64, true, false); break;
    case tile_cfg(32, 64, false): IBP_BODY(32, 64, false, false); break;
    case tile_cfg(32, 64, true): IBP_BODY(32, 64, true, false); break;
    case 8 | tile_cfg(128, 128, false): IBP_BODY(128, 128, false, true); break;
    case 8 | tile_cfg(128, 128, true): IBP_BODY(128, 128, true, true); break;
    case 8 | tile_cfg(128, 64, false): IBP_BODY(128, 64, false, true); break;
    case 8 | tile_cfg(128, 64, true): IBP_BODY(128, 64, true, true); break;
    case 8 | tile_cfg(64, 64, false): IBP_BODY(64, 64, false, true); break;
    case 8 | tile_cfg(64, 64, true): IBP_BODY(64, 64, true, true); break;
    case 8 | tile_cfg(32, 64, false): IBP_BODY(32, 64, false, true); break;
    default: IBP_BODY(32, 64, true, true); break;
  }
  #undef IBP_BODY
}

// The grouped kernel reads its table at offset 0 of the kernel-argument
// segment: it must stay the kernel's ONLY explicit argument (explicit
// arguments come first in the segment, hidden ones after), with the problem
// array leading the struct (asserted in conv_params.h).
static_assert(std::is_same<decltype(&conv_mfma_grouped_kernel<false>),
                           void (*)(ConvGroupParams)>::value &&
                  std::is_same<decltype(&conv_mfma_grouped_kernel<true>),
                               void (*)(ConvGroupParams)>::value,
              "conv_mfma_grouped_kernel must take the table as its only "
              "argument: it is read at kernarg offset 0");

// One output element of the split-K combine; slices summed s = 0..splitk-1
// from 0.f so the bits do not depend on which path ran.
__device__ __forceinline__ float combine_one(float v, float sc, float sh,
                                             bool has_scale, bool has_res,
                                             float r0, int act, bool has_rp,
                                             float r1, bool has_rp2, float r2) {
  if (has_scale) v = v * sc + sh;
  if (has_res) v += r0;
  if (act) v = leaky(v, 0.01f);
  if (has_rp) v += r1;
  if (has_rp2) v += r2;
  return v;
}

// split-K combine: y = act(scale*ws + shift (+res)) (+res_post...) -> bf16
// VEC: each thread owns 8 consecutive channels (C % 8 == 0, all pointers
// 16-byte aligned — host check): two 16-byte loads per slice, 16-byte
// scale/shift/residual loads, one 16-byte store. The channel-group index is
// walked incrementally, one 64-bit modulo per thread instead of per element.
// `bid` / `nblocks` are the block id and block count LOCAL to this problem
// (the grouped combine runs several problems in one grid).
//
// Output scatter (ConvParams::up): the slabs are in the problem's row order,
// y and the residuals are addressed at the row's full-resolution pixel. The
// host sets `up` only when the row count fits 32 bits.
__device__ __forceinline__ long long scatter_pixel(unsigned m,
                                                   const OutScatter& s) {
  const unsigned j = m % (unsigned)s.Wo; m /= (unsigned)s.Wo;
  const unsigned i = m % (unsigned)s.Ho;
  const unsigned n = m / (unsigned)s.Ho;
  return ((long long)n * (2 * s.Ho) + 2 * i + s.py) * (2 * s.Wo) + 2 * j + s.px;
}

template <bool VEC, bool UP>
__device__ __forceinline__ void splitk_combine_body(
    const float* __restrict__ ws, unsigned short* __restrict__ y,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const unsigned short* __restrict__ res,
    const unsigned short* __restrict__ res_post,
    const unsigned short* __restrict__ res_post2, long long total, int C,
    int act, int splitk, int bid, int nblocks, const OutScatter& os) {
  if constexpr (VEC) {
    const int C8 = C >> 3;
    const long long groups = total >> 3;
    const long long step = (long long)nblocks * blockDim.x;
    long long g = bid * (long long)blockDim.x + threadIdx.x;
    if (g >= groups) return;
    int c8 = (int)(g % C8);
    const int cstep = (int)(step % C8);
    // scattered output: the row index is walked beside the channel group
    unsigned row = UP ? (unsigned)(g / C8) : 0u;
    const unsigned rstep = UP ? (unsigned)(step / C8) : 0u;
    for (; g < groups; g += step) {
      const long long w = g << 3;
      const long long i = UP ? scatter_pixel(row, os) * C + c8 * 8 : w;
      floatx4 lo = floatx4{0.f, 0.f, 0.f, 0.f}, hi = lo;
      for (int s = 0; s < splitk; ++s) {
        const float* src = ws + (long long)s * total + w;
        lo += *reinterpret_cast<const floatx4*>(src);
        hi += *reinterpret_cast<const floatx4*>(src + 4);
      }
      floatx4 sc_lo = lo, sc_hi = lo, sh_lo = lo, sh_hi = lo;
      if (scale) {
        sc_lo = *reinterpret_cast<const floatx4*>(scale + c8 * 8);
        sc_hi = *reinterpret_cast<const floatx4*>(scale + c8 * 8 + 4);
        sh_lo = *reinterpret_cast<const floatx4*>(shift + c8 * 8);
        sh_hi = *reinterpret_cast<const floatx4*>(shift + c8 * 8 + 4);
      }
      ushortv8 r0 = ushortv8{0, 0, 0, 0, 0, 0, 0, 0}, r1 = r0, r2 = r0;
      if (res) r0 = *reinterpret_cast<const ushortv8*>(res + i);
      if (res_post) r1 = *reinterpret_cast<const ushortv8*>(res_post + i);
      if (res_post2) r2 = *reinterpret_cast<const ushortv8*>(res_post2 + i);
      ushortv8 out;
      #pragma unroll
      for (int e = 0; e < 4; ++e) {
        out[e] = f2us(combine_one(lo[e], sc_lo[e], sh_lo[e], scale != nullptr,
                                  res != nullptr, us2f(r0[e]), act,
                                  res_post != nullptr, us2f(r1[e]),
                                  res_post2 != nullptr, us2f(r2[e])));
        out[e + 4] = f2us(combine_one(
            hi[e], sc_hi[e], sh_hi[e], scale != nullptr, res != nullptr,
            us2f(r0[e + 4]), act, res_post != nullptr, us2f(r1[e + 4]),
            res_post2 != nullptr, us2f(r2[e + 4])));
      }
      *reinterpret_cast<ushortv8*>(y + i) = out;
      c8 += cstep;
      if (c8 >= C8) c8 -= C8;
      if constexpr (UP) {
        row += rstep;
        if (c8 < cstep) ++row;   // the channel group wrapped
      }
    }
  } else {
    for (long long w = bid * (long long)blockDim.x + threadIdx.x;
         w < total; w += (long long)nblocks * blockDim.x) {
      int c = (int)(w % C);
      const long long i =
          UP ? scatter_pixel((unsigned)(w / C), os) * C + c : w;
      float v = 0.f;
      for (int s = 0; s < splitk; ++s) v += ws[(long long)s * total + w];
      v = combine_one(v, scale ? scale[c] : 1.f, scale ? shift[c] : 0.f,
                      scale != nullptr, res != nullptr,
                      res ? us2f(res[i]) : 0.f, act, res_post != nullptr,
                      res_post ? us2f(res_post[i]) : 0.f,
                      res_post2 != nullptr,
                      res_post2 ? us2f(res_post2[i]) : 0.f);
      y[i] = f2us(v);
    }
  }
}

template <bool VEC>
__global__ void splitk_combine_kernel(const float* __restrict__ ws,
                                      unsigned short* __restrict__ y,
                                      const float* __restrict__ scale,
                                      const float* __restrict__ shift,
                                      const unsigned short* __restrict__ res,
                                      const unsigned short* __restrict__ res_post,
                                      const unsigned short* __restrict__ res_post2,
                                      long long total, int C, int act,
                                      int splitk) {
  splitk_combine_body<VEC, false>(ws, y, scale, shift, res, res_post,
                                  res_post2, total, C, act, splitk,
                                  (int)blockIdx.x, (int)gridDim.x,
                                  OutScatter{});
}

// grouped combine: the split members of one grouped conv launch, same
// block -> problem table scheme; each problem keeps the grid size and the
// <VEC> arithmetic it has alone.
template <bool UP>
__global__ void splitk_combine_grouped_kernel(CombineGroupParams g) {
  const int gb = blockIdx.x;
  int pi = 0, base = 0;
  #pragma unroll
  for (int i = 0; i < kMaxGroup - 1; ++i) {
    if (i + 1 < g.n && gb >= g.block_end[i]) {
      pi = i + 1;
      base = g.block_end[i];
    }
  }
  const CombineProblem& c = g.c[pi];
  const int nblocks = g.block_end[pi] - base;
  if (c.vec)
    splitk_combine_body<true, UP>(c.ws, c.y, c.scale, c.shift, c.res,
                                  c.res_post, c.res_post2, c.total, c.C,
                                  c.act, c.splitk, gb - base, nblocks, c.os);
  else
    splitk_combine_body<false, UP>(c.ws, c.y, c.scale, c.shift, c.res,
                                   c.res_post, c.res_post2, c.total, c.C,
                                   c.act, c.splitk, gb - base, nblocks, c.os);
}

// upfold weight pack: [Cout][Cin][3][3] -> [4][Cout][4*Cin], parity
// py*2+px outermost, then tap-major (a, b) with the channel fastest, like the
// forward pack. A 3x3 conv over a nearest-x2 image is, per output parity, a
// 2x2 conv over the low-resolution map whose weights are sums of 1, 2 or 4
// of the 3x3 weights: rows R(0,0)={0} R(0,1)={1,2} R(1,0)={0,1} R(1,1)={2}
// (same for columns). Summed in fp32 from 0.f, kh ascending then kw, rounded
// to bf16 once (round to nearest even).
__global__ void pack_upfold_weight_kernel(const unsigned short* __restrict__ w,
                                          unsigned short* __restrict__ out,
                                          int Cout, int Cin) {
  const long long per = (long long)Cout * 4 * Cin;
  const long long total = 4 * per;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    long long t = i / Cin;
    const int tap = (int)(t & 3); t >>= 2;
    const int co = (int)(t % Cout);
    const int par = (int)(t / Cout);
    const int py = par >> 1, px = par & 1, a = tap >> 1, b = tap & 1;
    // R(p, t) = [lo, hi]
    const int kh_lo = py == 0 ? a : 2 * a, kh_hi = py == 0 ? 2 * a : a + 1;
    const int kw_lo = px == 0 ? b : 2 * b, kw_hi = px == 0 ? 2 * b : b + 1;
    const unsigned short* src = w + ((long long)co * Cin + ci) * 9;
    float acc = 0.f;
    for (int kh = kh_lo; kh <= kh_hi; ++kh)
      for (int kw = kw_lo; kw <= kw_hi; ++kw) acc += us2f(src[kh * 3 + kw]);
    out[i] = f2us(acc);
  }
}

// two-source weight pack: 1x1 weights [Cout][Ca] and [Cout][Cb] -> one row
// [Cout][Ca + Cb] per output channel, source 1 first, each branch's
// per-channel scale (folded BN; absent = 1) multiplied in: float(w) *
// scale[co], one fp32 multiply, rounded to bf16 once (round to nearest even).
// The first Cout threads also write the fused shift shift_a + shift_b in
// fp32 (absent = 0).
__global__ void pack_cat_weight_kernel(const unsigned short* __restrict__ wa,
                                       const unsigned short* __restrict__ wb,
                                       const float* __restrict__ scale_a,
                                       const float* __restrict__ scale_b,
                                       const float* __restrict__ shift_a,
                                       const float* __restrict__ shift_b,
                                       unsigned short* __restrict__ out,
                                       float* __restrict__ shift_out,
                                       int Cout, int Ca, int Cb) {
  const int K = Ca + Cb;
  const long long total = (long long)Cout * K;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    const int co = (int)(i / K);
    const bool second = k >= Ca;
    const unsigned short w = second ? wb[(long long)co * Cb + (k - Ca)]
                                    : wa[(long long)co * Ca + k];
    const float* scale = second ? scale_b : scale_a;
    out[i] = f2us(us2f(w) * (scale ? scale[co] : 1.f));
    if (i < Cout)
      shift_out[i] = (shift_a ? shift_a[i] : 0.f) + (shift_b ? shift_b[i] : 0.f);
  }
}

// weight pack: [Cout,Cin,KH,KW] (standard contiguous) -> fwd [Cout][f*Cin+ci]
// and (optional) dgrad [Cin][(rot180 f)*Cout+co] in ONE pass. Weights change
// every optimizer step, so the eager flip/permute/reshape chains re-ran per
// layer per step (~500 small launches); this is one launch per weight.
__global__ void pack_weight_kernel(const unsigned short* __restrict__ w,
                                   unsigned short* __restrict__ fwd,
                                   unsigned short* __restrict__ dgr,
                                   int Cout, int Cin, int KH, int KW) {
  const long long total = (long long)Cout * Cin * KH * KW;
  const int KHW = KH * KW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int kw = (int)(i % KW);
    long long t = i / KW;
    const int kh = (int)(t % KH); t /= KH;
    const int ci = (int)(t % Cin);
    const int co = (int)(t / Cin);
    const unsigned short v = w[i];
    const int f = kh * KW + kw;
    fwd[(long long)co * KHW * Cin + f * Cin + ci] = v;
    if (dgr) {
      const int fr = (KH - 1 - kh) * KW + (KW - 1 - kw);
      dgr[(long long)ci * KHW * Cout + fr * Cout + co] = v;
    }
  }
}

}  // namespace ibp

// ===========================================================================
// Host side: tensors -> ConvProblem, outputs and workspaces, launches. What
// runs is decided in conv_plan.h (checked on the CPU, test_conv_plan_cpu.py).
using torch::Tensor;
using OptTensor = c10::optional<Tensor>;

void pack_conv_weight(const Tensor& w, Tensor& fwd_pack,
                      const OptTensor& dgrad_pack) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
              w.scalar_type() == at::ScalarType::BFloat16);
  int Cout = (int)w.size(0), Cin = (int)w.size(1);
  int KH = (int)w.size(2), KW = (int)w.size(3);
  auto stream = at::hip::getCurrentHIPStream().stream();
  dim3 grid(ibp::grid_1d(w.numel(), 256, 2048)), block(256);
  hipLaunchKernelGGL(
      ibp::pack_weight_kernel, grid, block, 0, stream,
      reinterpret_cast<const unsigned short*>(w.data_ptr()),
      reinterpret_cast<unsigned short*>(fwd_pack.data_ptr()),
      dgrad_pack.has_value()
          ? reinterpret_cast<unsigned short*>(dgrad_pack->data_ptr())
          : nullptr,
      Cout, Cin, KH, KW);
}

void pack_upfold_weight(const Tensor& w, Tensor& out) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.dim() == 4 &&
              w.scalar_type() == at::ScalarType::BFloat16 &&
              w.size(2) == 3 && w.size(3) == 3,
              "pack_upfold_weight: contiguous bf16 [Cout][Cin][3][3]");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
              out.scalar_type() == at::ScalarType::BFloat16 &&
              out.numel() == 16 * w.size(0) * w.size(1),
              "pack_upfold_weight: out must be bf16 [4][Cout][4*Cin]");
  auto stream = at::hip::getCurrentHIPStream().stream();
  dim3 grid(ibp::grid_1d(out.numel(), 256, 2048)), block(256);
  hipLaunchKernelGGL(ibp::pack_upfold_weight_kernel, grid, block, 0, stream,
                     reinterpret_cast<const unsigned short*>(w.data_ptr()),
                     reinterpret_cast<unsigned short*>(out.data_ptr()),
                     (int)w.size(0), (int)w.size(1));
}

// Weight pack and fused shift of a two-source 1x1 conv: out [Cout][Ca + Cb]
// bf16, shift_out [Cout] fp32 (pack_cat_weight_kernel). One launch.
void pack_cat_weight(const Tensor& wa, const Tensor& wb,
                     const OptTensor& scale_a, const OptTensor& scale_b,
                     const OptTensor& shift_a, const OptTensor& shift_b,
                     Tensor& out, Tensor& shift_out) {
  for (const Tensor* w : {&wa, &wb})
    TORCH_CHECK(w->is_cuda() && w->is_contiguous() && w->dim() == 4 &&
                w->scalar_type() == at::ScalarType::BFloat16 &&
                w->size(2) == 1 && w->size(3) == 1 && w->size(0) == wa.size(0),
                "pack_cat_weight: contiguous bf16 [Cout][C][1][1] weights "
                "with equal Cout");
  const int64_t Cout = wa.size(0), Ca = wa.size(1), Cb = wb.size(1);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
              out.scalar_type() == at::ScalarType::BFloat16 &&
              out.numel() == Cout * (Ca + Cb),
              "pack_cat_weight: out must be bf16 [Cout][Ca+Cb]");
  TORCH_CHECK(shift_out.is_cuda() && shift_out.is_contiguous() &&
              shift_out.scalar_type() == at::ScalarType::Float &&
              shift_out.numel() == Cout,
              "pack_cat_weight: shift_out must be fp32 [Cout]");
  auto vec = [&](const OptTensor& t) -> const float* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                t->scalar_type() == at::ScalarType::Float &&
                t->numel() == Cout,
                "pack_cat_weight: scales and shifts must be fp32 [Cout]");
    return t->data_ptr<float>();
  };
  auto stream = at::hip::getCurrentHIPStream().stream();
  dim3 grid(ibp::grid_1d(out.numel(), 256, 2048)), block(256);
  hipLaunchKernelGGL(ibp::pack_cat_weight_kernel, grid, block, 0, stream,
                     reinterpret_cast<const unsigned short*>(wa.data_ptr()),
                     reinterpret_cast<const unsigned short*>(wb.data_ptr()),
                     vec(scale_a), vec(scale_b), vec(shift_a), vec(shift_b),
                     reinterpret_cast<unsigned short*>(out.data_ptr()),
                     shift_out.data_ptr<float>(), (int)Cout, (int)Ca, (int)Cb);
}

namespace {

using ibp::ConvPlan;
using ibp::ConvProblem;

const unsigned short* bf16_ptr(const OptTensor& t) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::ScalarType::BFloat16,
              "conv_mfma: residuals must be bf16 device tensors");
  return reinterpret_cast<const unsigned short*>(t->data_ptr());
}

// One conv as the planner sees it, all but the output pointer: geom = {N, H,
// W, Cin, Cout, KH, KW, stride, pad_h, pad_w, dil_h, dil_w, Ho, Wo, zs}.
ConvProblem make_problem(const Tensor& x, const Tensor& w_packed,
                         const std::vector<int64_t>& geom,
                         const OptTensor& scale, const OptTensor& shift,
                         const OptTensor& residual, bool act,
                         const OptTensor& residual_post,
                         const OptTensor& residual_post2) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::ScalarType::BFloat16,
              "conv_mfma: x must be a bf16 device tensor");
  TORCH_CHECK(w_packed.is_contiguous(), "conv_mfma: pack must be contiguous");
  TORCH_CHECK(geom.size() == 15, "conv_mfma: geom needs 15 ints");
  ConvProblem q;
  ibp::ConvParams& p = q.p;
  int* const row[15] = {&p.N, &p.H, &p.W, &p.Cin, &p.Cout, &p.KH, &p.KW,
                        &p.stride, &p.pad_h, &p.pad_w, &p.dil_h, &p.dil_w,
                        &p.Ho, &p.Wo, &p.zs};
  for (int i = 0; i < 15; ++i) *row[i] = (int)geom[i];
  p.x = reinterpret_cast<const unsigned short*>(x.data_ptr());
  p.w = reinterpret_cast<const unsigned short*>(w_packed.data_ptr());
  p.scale = scale.has_value() ? scale->data_ptr<float>() : nullptr;
  p.shift = shift.has_value() ? shift->data_ptr<float>() : nullptr;
  p.res = bf16_ptr(residual);
  p.res_post = bf16_ptr(residual_post);
  p.res_post2 = bf16_ptr(residual_post2);
  p.act = act ? 1 : 0;
  return q;
}

// The second source of a two-source 1x1 conv: channels_last [N, Cin2, H, W]
// over x's pixels. geom's Cin stays the first source's; the planner checks
// the rest.
void set_second_source(ConvProblem& q, const Tensor& x, const Tensor& x2,
                       const Tensor& w_packed) {
  ibp::ConvParams& p = q.p;
  TORCH_CHECK(x2.is_cuda() && x2.device() == x.device() &&
              x2.scalar_type() == at::ScalarType::BFloat16 && x2.dim() == 4 &&
              x2.is_contiguous(at::MemoryFormat::ChannelsLast) &&
              x2.size(0) == p.N && x2.size(2) == p.H && x2.size(3) == p.W,
              "conv_mfma: x2 must be channels_last bf16 [N, Cin2, H, W]");
  TORCH_CHECK(x.dim() == 4 &&
              x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
              x.size(0) == p.N && x.size(1) == p.Cin && x.size(2) == p.H &&
              x.size(3) == p.W,
              "conv_mfma: with x2, x must be channels_last [N, Cin, H, W]");
  p.Cin2 = (int)x2.size(1);
  p.x2 = reinterpret_cast<const unsigned short*>(x2.data_ptr());
  TORCH_CHECK(w_packed.numel() == (int64_t)p.Cout * (p.Cin + p.Cin2),
              "conv_mfma: two-source pack must be [Cout][Cin + Cin2]");
}

Tensor alloc_output(ConvProblem& q, const Tensor& x) {
  Tensor y = torch::empty({q.p.N, q.p.Ho, q.p.Wo, q.p.Cout}, x.options());
  q.p.y = reinterpret_cast<unsigned short*>(y.data_ptr());
  return y;
}

// a runtime flag as a template argument: f(std::true_type{} / false_type{})
template <class F>
void with_flag(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// f(BM, BN, DEEP) with the plan's tile as integral constants
template <class F>
void with_tile(const ConvPlan& plan, F&& f) {
  using i128 = std::integral_constant<int, 128>;
  using i64 = std::integral_constant<int, 64>;
  using i32 = std::integral_constant<int, 32>;
  with_flag(plan.t.deep, [&](auto deep) {
    if (plan.t.BM == 128 && plan.t.BN == 128) f(i128{}, i128{}, deep);
    else if (plan.t.BM == 128) f(i128{}, i64{}, deep);
    else if (plan.t.BM == 64) f(i64{}, i64{}, deep);
    else f(i32{}, i64{}, deep);
  });
}

void launch_single(const ConvPlan& plan, hipStream_t stream) {
  const ibp::ConvParams& p = plan.p;
  TORCH_CHECK(!p.up, "upfold plans launch through the grouped kernel");
  with_tile(plan, [&](auto bm, auto bn, auto deep) {
    // the planner never sets the tap-uniform gather on a two-source conv
    TORCH_CHECK(!(p.Cin2 != 0 && p.gather != 0));
    with_flag(p.Cin2 != 0, [&](auto cat) {
      with_flag(p.gather != 0, [&](auto tu) {
        if constexpr (!(decltype(cat)::value && decltype(tu)::value))
          hipLaunchKernelGGL(
              (ibp::conv_mfma_kernel<decltype(bm)::value, decltype(bn)::value,
                                     decltype(deep)::value,
                                     decltype(cat)::value,
                                     decltype(tu)::value>),
              dim3(plan.nblocks), dim3(256), 0, stream, p);
      });
    });
  });
  if (p.splitk > 1)
    with_flag(plan.vec_combine, [&](auto vec) {
      hipLaunchKernelGGL(ibp::splitk_combine_kernel<decltype(vec)::value>,
                         dim3(ibp::combine_blocks(plan)), dim3(256), 0, stream,
                         p.ws, p.y, p.scale, p.shift, p.res, p.res_post,
                         p.res_post2, (long long)p.M * p.Cout, p.Cout, p.act,
                         p.splitk);
    });
}

void launch_group(const ibp::GroupPlan& gp, hipStream_t stream) {
  with_flag(gp.up, [&](auto up) {
    hipLaunchKernelGGL(ibp::conv_mfma_grouped_kernel<decltype(up)::value>,
                       dim3(gp.blocks), dim3(256), 0, stream, gp.g);
    if (gp.cg.n > 0)
      hipLaunchKernelGGL(
          ibp::splitk_combine_grouped_kernel<decltype(up)::value>,
          dim3(gp.cblocks), dim3(256), 0, stream, gp.cg);
  });
}

// Launch the plans in list order, at most kMaxGroup per launch: a chunk of one
// plain conv through its own kernel, with exactly its own workspace; every
// other chunk grouped, one shared workspace. Workspaces outlive the launches.
void run_plans(std::vector<ConvPlan>& plans, hipStream_t stream,
               const at::TensorOptions& f32) {
  std::vector<Tensor> keep;
  auto workspace = [&](long long elems) -> float* {
    if (elems <= 0) return nullptr;
    keep.push_back(torch::empty({elems}, f32));
    return keep.back().data_ptr<float>();
  };
  for (size_t first = 0; first < plans.size(); first += ibp::kMaxGroup) {
    const size_t last =
        std::min(plans.size(), first + (size_t)ibp::kMaxGroup);
    ConvPlan& head = plans[first];
    if (last - first == 1 && !head.p.up) {
      if (head.ws_elems > 0) ibp::set_workspace(head, workspace(head.ws_elems));
      launch_single(head, stream);
    } else {
      float* ws = workspace(ibp::group_workspace(plans, first, last));
      launch_group(ibp::assemble_group(plans, first, last, ws), stream);
    }
  }
}

}  // namespace

Tensor conv_mfma_fwd(const Tensor& x, const Tensor& w_packed,
                     const std::vector<int64_t>& geom, const OptTensor& scale,
                     const OptTensor& shift, const OptTensor& residual,
                     bool act, const OptTensor& residual_post,
                     const OptTensor& residual_post2, const OptTensor& x2) {
  ConvProblem q = make_problem(x, w_packed, geom, scale, shift, residual, act,
                               residual_post, residual_post2);
  // two-source 1x1 conv: K = Cin + Cin2, w_packed [Cout][Cin + Cin2]
  if (x2.has_value()) set_second_source(q, x, *x2, w_packed);
  Tensor y = alloc_output(q, x);
  std::vector<ConvPlan> plans{ibp::plan_conv(q)};
  run_plans(plans, at::hip::getCurrentHIPStream().stream(),
            x.options().dtype(torch::kFloat32));
  return y;
}

// Several independent convs in as few launches as possible: lists of the
// conv_mfma_fwd arguments, outputs in list order. Every member keeps the plan
// it gets alone — same tile, split, epilogue path and summation order — so
// each output is bit-identical to the single call.
std::vector<Tensor> conv_mfma_fwd_grouped(
    const std::vector<Tensor>& xs, const std::vector<Tensor>& ws_packed,
    const std::vector<std::vector<int64_t>>& geom,
    const std::vector<OptTensor>& scales, const std::vector<OptTensor>& shifts,
    const std::vector<OptTensor>& residuals, const std::vector<bool>& acts,
    const std::vector<OptTensor>& residual_posts,
    const std::vector<OptTensor>& residual_post2s) {
  const size_t n = xs.size();
  TORCH_CHECK(n > 0 && ws_packed.size() == n && geom.size() == n &&
              scales.size() == n && shifts.size() == n &&
              residuals.size() == n && acts.size() == n &&
              residual_posts.size() == n && residual_post2s.size() == n,
              "conv_mfma_fwd_grouped: argument lists differ in length");
  std::vector<ConvPlan> plans;
  std::vector<Tensor> ys;
  plans.reserve(n);
  ys.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(xs[i].device() == xs[0].device());
    ConvProblem q = make_problem(xs[i], ws_packed[i], geom[i], scales[i],
                                 shifts[i], residuals[i], acts[i],
                                 residual_posts[i], residual_post2s[i]);
    ys.push_back(alloc_output(q, xs[i]));
    plans.push_back(ibp::plan_conv(q));
  }
  run_plans(plans, at::hip::getCurrentHIPStream().stream(),
            xs[0].options().dtype(torch::kFloat32));
  return ys;
}

// y[N, 2H, 2W, Cout] = epilogue(conv3x3(nearest_x2(x_low), W, pad 1)) as
// four stride-1 2x2 convs over x_low [N, H, W, Cin], one per output parity
// (py, px), with pad (1-py, 1-px) and the folded weights of
// pack_upfold_weight; each stores into its own pixels of the shared output.
// geom is the layer's row: 3x3 over H x W = the LOW resolution, Ho x Wo =
// 2H x 2W. One grouped conv launch, at most one grouped combine.
Tensor conv_mfma_upfold_fwd(const Tensor& x_low, const Tensor& packs,
                            const std::vector<int64_t>& geom,
                            const OptTensor& scale, const OptTensor& shift,
                            bool act, const OptTensor& residual_post,
                            const OptTensor& residual_post2) {
  ConvProblem q = make_problem(x_low, packs, geom, scale, shift, c10::nullopt,
                               act, residual_post, residual_post2);
  ibp::ConvParams& p = q.p;
  const int64_t N = p.N, H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout;
  TORCH_CHECK(p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad_h == 1 &&
              p.pad_w == 1 && p.dil_h == 1 && p.dil_w == 1 && p.zs == 1 &&
              p.Ho == 2 * H && p.Wo == 2 * W,
              "conv_mfma_upfold_fwd: geom must be a 3x3 stride-1 pad-1 conv "
              "with Ho x Wo = 2H x 2W");
  TORCH_CHECK(x_low.is_contiguous() && x_low.numel() == N * H * W * Cin,
              "conv_mfma_upfold_fwd: x_low must be contiguous [N][H][W][Cin]");
  TORCH_CHECK(packs.is_cuda() &&
              packs.scalar_type() == at::ScalarType::BFloat16 &&
              packs.numel() == 16 * Cout * Cin,
              "conv_mfma_upfold_fwd: packs must be bf16 [4][Cout][4*Cin]");
  for (const auto* r : {&residual_post, &residual_post2})
    TORCH_CHECK(!r->has_value() || (*r)->numel() == 4 * N * H * W * Cout,
                "conv_mfma_upfold_fwd: residuals must be bf16 "
                "[N][2H][2W][Cout]");
  Tensor y = alloc_output(q, x_low);
  // each parity: a 2x2 conv whose rows index the low-resolution grid
  p.KH = p.KW = 2;
  p.Ho = p.H;
  p.Wo = p.W;
  p.up = 1;
  q.tile = ibp::plan_upfold_tile(N * H * W, p.Cout, p.Cin);
  std::vector<ConvPlan> plans;
  plans.reserve(4);
  for (int par = 0; par < 4; ++par) {
    p.py = par >> 1;
    p.px = par & 1;
    p.pad_h = 1 - p.py;
    p.pad_w = 1 - p.px;
    p.w = reinterpret_cast<const unsigned short*>(packs.data_ptr()) +
          (long long)par * Cout * 4 * Cin;
    plans.push_back(ibp::plan_conv(q));
  }
  run_plans(plans, at::hip::getCurrentHIPStream().stream(),
            x_low.options().dtype(torch::kFloat32));
  return y;
}

// {BM, BN, splitk, deep} that a conv with these GEMM extents is planned with
// (M = N*Ho*Wo, K = KH*KW*Cin) — lets tests assert which tile and split a
// shape lands on.
std::vector<int64_t> conv_mfma_tile_plan(int64_t M, int64_t Cout, int64_t K) {
  const ibp::TilePlan t = ibp::plan_tile(M, (int)Cout, (int)K);
  return {t.BM, t.BN, t.splitk, t.deep ? 1 : 0};
}

// {BM, BN, splitk, deep, gather} of the plan that conv_mfma_fwd(x, w_packed,
// geom, ...) runs: the gather depends on the operands' addresses as well as
// on the geometry (conv_plan.h, gather_eligible). Launches nothing.
std::vector<int64_t> conv_mfma_conv_plan(const Tensor& x,
                                         const Tensor& w_packed,
                                         const std::vector<int64_t>& geom) {
  const ConvProblem q =
      make_problem(x, w_packed, geom, c10::nullopt, c10::nullopt, c10::nullopt,
                   false, c10::nullopt, c10::nullopt);
  const ConvPlan plan = ibp::plan_conv(q);
  return {plan.t.BM, plan.t.BN, plan.p.splitk, plan.t.deep ? 1 : 0,
          plan.p.gather};
}

// {BM, BN, splitk, deep} shared by the four parities of an upfold conv over
// M_low = N*H*W low-resolution pixels.
std::vector<int64_t> conv_mfma_upfold_plan(int64_t M_low, int64_t Cout,
                                           int64_t Cin) {
  const ibp::TilePlan t = ibp::plan_upfold_tile(M_low, (int)Cout, (int)Cin);
  return {t.BM, t.BN, t.splitk, t.deep ? 1 : 0};
}
