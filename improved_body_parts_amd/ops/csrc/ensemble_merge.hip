// Fused tail of the rotation-free ensemble forward.
//
// After the network forward, predict() runs ~10 eager ops per image: flip the
// mirrored view back, permute its L/R channels, average the two views, bicubic
// x-stride upsample to the padded size, crop the padding, bicubic resize to the
// original size, divide by the number of ensemble runs and accumulate. All of
// it is one separable linear map of the stride-resolution output, so it runs
// here as a single pass:
//
//   acc[n,c,y,x] (+)= scale * sum_k sum_l Ry[y,k] * Rx[x,l] *
//       0.5 * (V[n, cm[c], ys[y]+k, xs[x]+l] + V[N+n, cf[c], ys[y]+k, w4-1-(xs[x]+l)])
//
// Ry/Rx are the per-axis compositions (resize . crop . upsample) built on the
// host as (start, weights[K]) tap tables; cm/cf gather the output channel order
// out of the network's channel order for the plain and the mirrored view.
//
// Work split: one block owns a TY x TX output tile of CB channels of one image.
//   1. stage the flip-merged source window of the tile into LDS (lanes along the
//      NHWC channel axis of the source, several pixels' loads in flight),
//   2. per channel (one per wave, waves run independently): horizontal pass
//      window -> the wave's LDS row buffer, vertical pass row buffer ->
//      registers -> planar fp32 store with the 64 lanes of the wave along x
//      (256-byte rows).
// Every output element is written by exactly one thread and nothing is atomic,
// so the result is bitwise repeatable.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace ibp {

constexpr int kEmTX = 64;      // output columns per block (= lanes of a wave)
constexpr int kEmTY = 16;      // output rows per block
constexpr int kEmWaves = 4;    // channels in flight per block
constexpr int kEmK = 8;        // tap-table row pitch (weights padded with 0)
constexpr int kEmStageC = 32;  // staging lanes along the channel axis (>= CB)
constexpr int kEmStageU = 4;   // staging passes in flight
constexpr int kEmVU = 8;       // output rows in flight in the vertical pass

// Orders a wave's LDS writes before its later LDS reads (and the reverse). The
// row buffer of the channel loop is private to its wave, and a wave's LDS
// operations execute in issue order, so a block barrier is not needed there; a
// __syncthreads() would also wait for the wave's outstanding global stores.
// Only the LDS counter is waited for: a fence would drain the stores too.
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// KT: taps actually walked per axis (the real span of the tables, <= kEmK).
template <typename T, int KT>
__global__ void __launch_bounds__(kEmTX * kEmWaves)
ensemble_merge_kernel(const T* __restrict__ src,        // [2N][h4][w4][Cs]
                      const int* __restrict__ chan_main,  // [C]
                      const int* __restrict__ chan_flip,  // [C]
                      const int* __restrict__ ystart,     // [H]
                      const float* __restrict__ yw,       // [H][kEmK]
                      const int* __restrict__ xstart,     // [W]
                      const float* __restrict__ xw,       // [W][kEmK]
                      float* __restrict__ out,            // [N][C][H][W]
                      int N, int C, int Cs, int h4, int w4, int H, int W,
                      int CB, int WR, int WC, int plane_pitch,
                      float scale, int accumulate) {
  extern __shared__ float em_lds[];
  float* win = em_lds;                           // [CB][plane_pitch]
  float* rowbuf = em_lds + CB * plane_pitch;     // [kEmWaves][WR][kEmTX]

  const int groups = (C + CB - 1) / CB;
  const int n = blockIdx.z / groups;
  const int c0 = (blockIdx.z % groups) * CB;
  const int cb = min(CB, C - c0);
  const int x0 = blockIdx.x * kEmTX;
  const int y0 = blockIdx.y * kEmTY;
  const int ys0 = ystart[y0];
  const int xs0 = xstart[x0];

  // ---- 1. stage 0.5 * (view + mirrored view) of the source window ----------
  // 32 lanes walk the channels of one source pixel (its NHWC line), 8 pixels
  // per pass; four passes of loads are issued before the first is consumed.
  const long long img = (long long)h4 * w4 * Cs;
  const T* v0 = src + (long long)n * img;
  const T* v1 = src + (long long)(N + n) * img;
  {
    const int c = threadIdx.x & (kEmStageC - 1);
    const int p0 = threadIdx.x / kEmStageC;
    constexpr int kPix = kEmTX * kEmWaves / kEmStageC;   // pixels per pass
    const int npix = WR * WC;
    if (c < cb) {
      const int cm = chan_main[c0 + c], cf = chan_flip[c0 + c];
      float* wp = win + c * plane_pitch;
      for (int pb = p0; pb < npix; pb += kPix * kEmStageU) {
        float va[kEmStageU], vb[kEmStageU];
        #pragma unroll
        for (int u = 0; u < kEmStageU; ++u) {
          const int p = pb + u * kPix;
          const int r = p / WC;
          const int rr = ys0 + r, ss = xs0 + (p - r * WC);
          const bool ok = p < npix && rr >= 0 && rr < h4 && ss >= 0 && ss < w4;
          const long long row = (long long)(ok ? rr : 0) * w4;
          const int sc = ok ? ss : 0;
          // always load (from pixel 0 when outside) and select afterwards: a
          // load under a per-lane condition is waited for on the spot
          const float ta = ldf(v0 + (row + sc) * Cs + cm);
          const float tb = ldf(v1 + (row + (w4 - 1 - sc)) * Cs + cf);
          va[u] = ok ? ta : 0.f;
          vb[u] = ok ? tb : 0.f;
        }
        #pragma unroll
        for (int u = 0; u < kEmStageU; ++u) {
          const int p = pb + u * kPix;
          if (p < npix) wp[p] = 0.5f * (va[u] + vb[u]);
        }
      }
    }
  }

  // ---- per-thread column taps (x is fixed for the whole block) -------------
  const int lane = threadIdx.x & (kEmTX - 1);
  const int wave = threadIdx.x / kEmTX;
  const int x = x0 + lane;
  const int xc = min(x, W - 1);
  float wx[KT];
  #pragma unroll
  for (int l = 0; l < KT; ++l) wx[l] = xw[(long long)xc * kEmK + l];
  // window offsets are clamped so that no tap can leave the staged window,
  // whatever the tables hold (the host sizes WR/WC from the same tables)
  const int ox = min(max(xstart[xc] - xs0, 0), WC - KT);
  const int ny = min(kEmTY, H - y0);
  float* rb = rowbuf + wave * WR * kEmTX;
  __syncthreads();

  // ---- 2. one channel per wave: horizontal pass, then vertical pass --------
  for (int cc = 0; cc < cb; cc += kEmWaves) {
    const int c = cc + wave;
    if (c < cb) {
      const float* pl = win + c * plane_pitch + ox;
      for (int r = 0; r < WR; ++r) {
        float a = 0.f;
        #pragma unroll
        for (int l = 0; l < KT; ++l) a += wx[l] * pl[r * WC + l];
        rb[r * kEmTX + lane] = a;
      }
    }
    wave_lds_sync();
    if (c < cb && x < W) {
      float* op = out + (((long long)n * C + c0 + c) * H + y0) * W + x;
      // kEmVU rows at a time: all their previous values are requested before
      // any is needed, and their stores leave together
      #pragma unroll 1
      for (int j0 = 0; j0 < ny; j0 += kEmVU) {
        float a[kEmVU];
        #pragma unroll
        for (int u = 0; u < kEmVU; ++u) a[u] = 0.f;
        if (accumulate) {
          #pragma unroll
          for (int u = 0; u < kEmVU; ++u)   // rows past the tile re-read its last
            a[u] = op[(long long)min(j0 + u, ny - 1) * W];
        }
        #pragma unroll
        for (int u = 0; u < kEmVU; ++u) {
          const int y = min(y0 + j0 + u, H - 1);
          const int oy = min(max(ystart[y] - ys0, 0), WR - KT);
          const float* wy = yw + (long long)y * kEmK;
          float t = 0.f;
          #pragma unroll
          for (int k = 0; k < KT; ++k) t += wy[k] * rb[(oy + k) * kEmTX + lane];
          a[u] += scale * t;
        }
        #pragma unroll
        for (int u = 0; u < kEmVU; ++u)
          if (j0 + u < ny) op[(long long)(j0 + u) * W] = a[u];
      }
    }
    wave_lds_sync();
  }
}

}  // namespace ibp

using torch::Tensor;

// src: (2N, h4, w4, Cs) contiguous (the NHWC memory of the model output);
// out: (N, C, H, W) fp32 contiguous. cb/wr/wc: channels per block and the source
// window extent per tile, sized by the host from the tap tables; span: real taps.
void ensemble_merge(const Tensor& src, const Tensor& chan_main,
                    const Tensor& chan_flip, const Tensor& ystart,
                    const Tensor& yw, const Tensor& xstart, const Tensor& xw,
                    Tensor& out, double scale, bool accumulate, int64_t cb,
                    int64_t wr, int64_t wc, int64_t span) {
  TORCH_CHECK(src.is_cuda() && out.is_cuda(), "ensemble_merge: GPU tensors only");
  TORCH_CHECK(src.dim() == 4 && src.is_contiguous(),
              "ensemble_merge: src must be contiguous (2N, h4, w4, C)");
  TORCH_CHECK(out.dim() == 4 && out.is_contiguous() &&
              out.scalar_type() == at::kFloat,
              "ensemble_merge: out must be contiguous fp32 (N, C, H, W)");
  const int N = (int)out.size(0), C = (int)out.size(1);
  const int H = (int)out.size(2), W = (int)out.size(3);
  const int h4 = (int)src.size(1), w4 = (int)src.size(2), Cs = (int)src.size(3);
  TORCH_CHECK(src.size(0) == 2 * (int64_t)N, "ensemble_merge: src holds 2N views");
  auto is_i32 = [&](const Tensor& t, int64_t n) {
    return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kInt &&
           t.numel() == n;
  };
  auto is_f32 = [&](const Tensor& t, int64_t n) {
    return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat &&
           t.numel() == n;
  };
  TORCH_CHECK(is_i32(chan_main, C) && is_i32(chan_flip, C),
              "ensemble_merge: channel tables must be int32 [C]");
  TORCH_CHECK(is_i32(ystart, H) && is_f32(yw, (int64_t)H * ibp::kEmK) &&
              is_i32(xstart, W) && is_f32(xw, (int64_t)W * ibp::kEmK),
              "ensemble_merge: tap tables must be int32 [n] / fp32 [n][8]");
  TORCH_CHECK(span >= 1 && span <= ibp::kEmK, "ensemble_merge: span out of range");
  const int KT = span <= 5 ? 5 : ibp::kEmK;
  TORCH_CHECK(cb >= 1 && cb <= C && cb <= ibp::kEmStageC && wr >= KT && wc >= KT,
              "ensemble_merge: bad tile plan");
  if (N == 0 || H == 0 || W == 0) return;

  const int plane_pitch = (int)(wr * wc) | 1;   // odd pitch: channel-major writes
  const size_t lds = ((size_t)cb * plane_pitch +
                      (size_t)ibp::kEmWaves * wr * ibp::kEmTX) * sizeof(float);
  TORCH_CHECK(lds <= 64 * 1024, "ensemble_merge: tile plan needs ", lds,
              " bytes of LDS");
  const int groups = (C + (int)cb - 1) / (int)cb;
  dim3 block(ibp::kEmTX * ibp::kEmWaves);
  dim3 grid((W + ibp::kEmTX - 1) / ibp::kEmTX, (H + ibp::kEmTY - 1) / ibp::kEmTY,
            N * groups);
  TORCH_CHECK(grid.y <= 65535 && grid.z <= 65535, "ensemble_merge: grid too large");
  hipStream_t stream = at::hip::getCurrentHIPStream().stream();

  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::BFloat16, at::ScalarType::Half,
      src.scalar_type(), "ensemble_merge", [&] {
    auto launch = [&](auto kt) {
      constexpr int kKT = decltype(kt)::value;
      hipLaunchKernelGGL((ibp::ensemble_merge_kernel<scalar_t, kKT>), grid, block,
                         lds, stream,
                         reinterpret_cast<const scalar_t*>(src.data_ptr()),
                         chan_main.data_ptr<int>(), chan_flip.data_ptr<int>(),
                         ystart.data_ptr<int>(), yw.data_ptr<float>(),
                         xstart.data_ptr<int>(), xw.data_ptr<float>(),
                         out.data_ptr<float>(), N, C, Cs, h4, w4, H, W, (int)cb,
                         (int)wr, (int)wc, plane_pitch, (float)scale,
                         accumulate ? 1 : 0);
    };
    if (KT == 5) launch(std::integral_constant<int, 5>{});
    else launch(std::integral_constant<int, ibp::kEmK>{});
  });
  IBP_CHECK_HIP(hipGetLastError());
}
