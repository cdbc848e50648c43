// Device-side training augmentation: batched affine warp over ragged sources.
//
// Device twin of data/transformer.py::Transformer.warp. One launch turns a
// batch of raw uint8 records of different sizes into the network's input image
// (NHWC, [0,1], optionally tinted) and the two stride-grid masks:
//
//   (sx, sy) = Mi . (ox, oy, 1)                    Mi: destination -> source
//   outside [0, Ws-1] x [0, Hs-1]  -> the constant (128 / 1.0 / 0.0)
//   otherwise                      -> bilinear blend of the four neighbours
//
// which is scipy.ndimage.affine_transform(order=1, mode="constant"): no
// blending toward the constant at the border. The masks are warped at full
// resolution and averaged over their stride x stride cell in registers; no
// full-resolution mask is ever written.
//
// Sources are read with direct loads, not staged in LDS. A tile's source
// footprint is a rotated, per-sample-scaled rectangle of 3-byte pixels: its
// bounding box has no fixed size, a zoomed-out sample would not fit, and the
// staging copy would be as unaligned as the gather itself. One image's working
// set (<= 1 MB) stays in L2, so the neighbours are fetched from there: the two
// horizontally adjacent pixels of a row (6 bytes) as ONE unaligned 8-byte
// load, two loads per output pixel instead of twelve byte loads. The packer
// pads every source so the 2 spare bytes never leave the buffer.
//
// Grid: blockIdx.y = sample, so the descriptor is block-uniform (scalar
// loads); the first `img_blocks` blocks of a sample own four consecutive image
// pixels per thread (three 16-byte stores in fp32, three 8-byte stores in
// bf16), the rest own one mask cell per thread and hand their results to every
// fourth lane for a 16-byte store. One thread owns each output element and
// nothing is atomic, so the result is bitwise repeatable.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace ibp {

constexpr int kAugBlock = 256;
constexpr int kAugPX = 4;       // image pixels per thread
constexpr int kAugSlack = 8;    // bytes the packer leaves readable past a source

// One row of the descriptor table; the packer (ops/augment.py) writes the
// same layout as a numpy structured dtype.
struct AugDesc {
  long long img_off;    // byte offset of the (Hs, Ws, 3) uint8 image
  long long mask_off;   // byte offset of the (2, Hs, Ws) mask pair
  int hs, ws;
  float mi[6];          // inverse affine, row-major 2x3
  float mask_scale[2];  // 1 or 1/255 for mask_miss, mask_all
  float gain[3];
  float shift;
  int flags;            // bit 0: tint, bit 1: masks are float32 (else uint8)
  int pad;
};
static_assert(sizeof(AugDesc) == 80, "descriptor layout is shared with Python");

__device__ __forceinline__ unsigned long long ld_u64_unaligned(const uint8_t* p) {
  unsigned long long v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// Source coordinate -> clamped neighbour indices, weights and the inside test.
struct AugTap {
  int x0, y0, y1;
  float fx, fy;
  bool inside;
};

__device__ __forceinline__ AugTap aug_tap(const float* mi, int ox, int oy,
                                          int ws, int hs) {
  const float sx = (mi[0] * (float)ox + mi[1] * (float)oy) + mi[2];
  const float sy = (mi[3] * (float)ox + mi[4] * (float)oy) + mi[5];
  AugTap t;
  t.inside = sx >= 0.f && sx <= (float)(ws - 1) && sy >= 0.f && sy <= (float)(hs - 1);
  const float flx = floorf(sx), fly = floorf(sy);
  // always clamped: a coordinate outside (or NaN) still addresses the source
  t.x0 = min(max((int)flx, 0), ws - 1);
  t.y0 = min(max((int)fly, 0), hs - 1);
  t.y1 = min(t.y0 + 1, hs - 1);
  t.fx = sx - flx;
  t.fy = sy - fly;
  return t;
}

__device__ __forceinline__ float aug_blend(float a, float b, float c, float d,
                                           float fx, float fy) {
  const float top = (1.f - fx) * a + fx * b;
  const float bot = (1.f - fx) * c + fx * d;
  return (1.f - fy) * top + fy * bot;
}

__device__ __forceinline__ void aug_store(float* p, const float (&o)[12]) {
  float4* q = reinterpret_cast<float4*>(p);
  q[0] = make_float4(o[0], o[1], o[2], o[3]);
  q[1] = make_float4(o[4], o[5], o[6], o[7]);
  q[2] = make_float4(o[8], o[9], o[10], o[11]);
}
__device__ __forceinline__ void aug_store(unsigned short* p, const float (&o)[12]) {
  uint2* q = reinterpret_cast<uint2*>(p);
  #pragma unroll
  for (int k = 0; k < 3; ++k) {
    uint2 v;
    v.x = (unsigned)f2us(o[4 * k + 0]) | ((unsigned)f2us(o[4 * k + 1]) << 16);
    v.y = (unsigned)f2us(o[4 * k + 2]) | ((unsigned)f2us(o[4 * k + 3]) << 16);
    q[k] = v;
  }
}

template <typename OutT>
__global__ void __launch_bounds__(kAugBlock)
augment_warp_kernel(const uint8_t* __restrict__ src,      // packed records
                    const AugDesc* __restrict__ desc,     // [B]
                    OutT* __restrict__ img_out,           // [B][H][W][3]
                    float* __restrict__ miss_out,         // [B][h][w]
                    float* __restrict__ all_out,          // [B][h][w]
                    int H, int W, int h, int w, int stride, int img_blocks) {
  const int b = blockIdx.y;
  const AugDesc d = desc[b];
  const int hs = d.hs, ws = d.ws;

  if ((int)blockIdx.x < img_blocks) {
    // ---- image: four consecutive output pixels of one row per thread -------
    const int wq = W / kAugPX;
    const int t = blockIdx.x * kAugBlock + threadIdx.x;
    if (t >= H * wq) return;
    const int oy = t / wq;
    const int ox0 = (t - oy * wq) * kAugPX;
    const uint8_t* im = src + d.img_off;

    AugTap tap[kAugPX];
    unsigned long long r0[kAugPX], r1[kAugPX];
    #pragma unroll
    for (int u = 0; u < kAugPX; ++u) {
      tap[u] = aug_tap(d.mi, ox0 + u, oy, ws, hs);
      // pixels x0 and x0+1 of a row are 6 adjacent bytes; at x0 = Ws-1 the
      // second one is not a neighbour, and its weight fx is exactly 0 there
      r0[u] = ld_u64_unaligned(im + ((long long)tap[u].y0 * ws + tap[u].x0) * 3);
      r1[u] = ld_u64_unaligned(im + ((long long)tap[u].y1 * ws + tap[u].x0) * 3);
    }
    const bool tint = d.flags & 1;
    float o[kAugPX * 3];
    #pragma unroll
    for (int u = 0; u < kAugPX; ++u) {
      #pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = (float)((r0[u] >> (8 * c)) & 0xffu);
        const float bb = (float)((r0[u] >> (8 * (c + 3))) & 0xffu);
        const float cc = (float)((r1[u] >> (8 * c)) & 0xffu);
        const float dd = (float)((r1[u] >> (8 * (c + 3))) & 0xffu);
        float v = aug_blend(a, bb, cc, dd, tap[u].fx, tap[u].fy);
        v = (tap[u].inside ? v : 128.f) / 255.f;
        if (tint) v = fminf(fmaxf(v * d.gain[c] + d.shift, 0.f), 1.f);
        o[u * 3 + c] = v;
      }
    }
    aug_store(img_out + (((long long)b * H + oy) * W + ox0) * 3, o);
    return;
  }

  // ---- masks: one stride-grid cell per thread, both masks at once ----------
  const int cells = h * w;
  const int t = ((int)blockIdx.x - img_blocks) * kAugBlock + threadIdx.x;
  const bool live = t < cells;
  const int tc = live ? t : cells - 1;   // idle lanes stay for the shuffles
  const int cy = tc / w, cx = tc - cy * w;
  const bool f32 = d.flags & 2;
  const uint8_t* mk = src + d.mask_off;
  const long long plane = (long long)hs * ws;
  const float s0 = d.mask_scale[0], s1 = d.mask_scale[1];

  float acc_miss = 0.f, acc_all = 0.f;
  for (int j = 0; j < stride; ++j) {
    for (int i = 0; i < stride; ++i) {
      const AugTap tp = aug_tap(d.mi, cx * stride + i, cy * stride + j, ws, hs);
      const long long p0 = (long long)tp.y0 * ws + tp.x0;
      const long long p1 = (long long)tp.y1 * ws + tp.x0;
      float m[2][4];
      if (f32) {
        #pragma unroll
        for (int k = 0; k < 2; ++k) {
          float2 top, bot;
          __builtin_memcpy(&top, mk + (k * plane + p0) * 4, 8);
          __builtin_memcpy(&bot, mk + (k * plane + p1) * 4, 8);
          // at x0 = Ws-1 the second float is not a neighbour (weight 0); it
          // may be padding, so it must not reach the blend as a NaN
          const bool last = tp.x0 == ws - 1;
          m[k][0] = top.x; m[k][1] = last ? top.x : top.y;
          m[k][2] = bot.x; m[k][3] = last ? bot.x : bot.y;
        }
      } else {
        #pragma unroll
        for (int k = 0; k < 2; ++k) {
          unsigned short top, bot;
          __builtin_memcpy(&top, mk + k * plane + p0, 2);
          __builtin_memcpy(&bot, mk + k * plane + p1, 2);
          m[k][0] = (float)(top & 0xffu); m[k][1] = (float)(top >> 8);
          m[k][2] = (float)(bot & 0xffu); m[k][3] = (float)(bot >> 8);
        }
      }
      const float vm = aug_blend(m[0][0] * s0, m[0][1] * s0, m[0][2] * s0,
                                 m[0][3] * s0, tp.fx, tp.fy);
      const float va = aug_blend(m[1][0] * s1, m[1][1] * s1, m[1][2] * s1,
                                 m[1][3] * s1, tp.fx, tp.fy);
      acc_miss += tp.inside ? vm : 1.f;
      acc_all += tp.inside ? va : 0.f;
    }
  }
  const float inv = (float)(stride * stride);
  const float vm = acc_miss / inv, va = acc_all / inv;
  float* mo = miss_out + (long long)b * cells;
  float* ao = all_out + (long long)b * cells;
  if ((w & 3) == 0) {
    // four neighbouring lanes hold four neighbouring cells of one row
    const float m1 = __shfl_down(vm, 1, 64), m2 = __shfl_down(vm, 2, 64),
                m3 = __shfl_down(vm, 3, 64);
    const float a1 = __shfl_down(va, 1, 64), a2 = __shfl_down(va, 2, 64),
                a3 = __shfl_down(va, 3, 64);
    if (live && (threadIdx.x & 3) == 0) {
      *reinterpret_cast<float4*>(mo + t) = make_float4(vm, m1, m2, m3);
      *reinterpret_cast<float4*>(ao + t) = make_float4(va, a1, a2, a3);
    }
  } else if (live) {
    mo[t] = vm;
    ao[t] = va;
  }
}

}  // namespace ibp

using torch::Tensor;

// packed: 1-D uint8 buffer of every sample's image and mask pair; desc: (B, 80)
// uint8 rows of ibp::AugDesc. The caller has checked on the host that every
// source, plus kAugSlack bytes, lies inside `packed` (ops/augment.py).
std::vector<Tensor> augment_warp(const Tensor& packed, const Tensor& desc,
                                 int64_t H, int64_t W, int64_t stride,
                                 bool bf16_out) {
  TORCH_CHECK(packed.is_cuda() && packed.dim() == 1 && packed.is_contiguous() &&
              packed.scalar_type() == at::kByte,
              "augment_warp: packed must be a contiguous 1-D uint8 GPU tensor");
  TORCH_CHECK(desc.is_cuda() && desc.dim() == 2 && desc.is_contiguous() &&
              desc.scalar_type() == at::kByte &&
              desc.size(1) == (int64_t)sizeof(ibp::AugDesc),
              "augment_warp: desc must be a contiguous (B, 80) uint8 GPU tensor");
  TORCH_CHECK(desc.device() == packed.device(), "augment_warp: device mismatch");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(desc.data_ptr()) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(packed.data_ptr()) % 16 == 0,
              "augment_warp: misaligned buffers");
  TORCH_CHECK(stride >= 1 && H >= stride && W >= stride && W % ibp::kAugPX == 0,
              "augment_warp: output width must be a multiple of 4");
  TORCH_CHECK(H * W < (1LL << 30), "augment_warp: output too large");
  const int64_t B = desc.size(0);
  const int64_t h = H / stride, w = W / stride;
  TORCH_CHECK(B <= 65535, "augment_warp: batch too large");

  auto fopt = packed.options().dtype(torch::kFloat32);
  Tensor img = torch::empty({B, H, W, 3},
                            bf16_out ? fopt.dtype(torch::kBFloat16) : fopt);
  Tensor miss = torch::empty({B, h, w}, fopt);
  Tensor all = torch::empty({B, h, w}, fopt);
  if (B == 0) return {img, miss, all};

  const int img_blocks =
      (int)((H * (W / ibp::kAugPX) + ibp::kAugBlock - 1) / ibp::kAugBlock);
  const int mask_blocks = (int)((h * w + ibp::kAugBlock - 1) / ibp::kAugBlock);
  dim3 block(ibp::kAugBlock), grid(img_blocks + mask_blocks, (unsigned)B);
  hipStream_t stream = at::hip::getCurrentHIPStream().stream();
  const uint8_t* src = packed.data_ptr<uint8_t>();
  const auto* dp = reinterpret_cast<const ibp::AugDesc*>(desc.data_ptr());
  if (bf16_out) {
    hipLaunchKernelGGL((ibp::augment_warp_kernel<unsigned short>), grid, block, 0,
                       stream, src, dp,
                       reinterpret_cast<unsigned short*>(img.data_ptr()),
                       miss.data_ptr<float>(), all.data_ptr<float>(), (int)H,
                       (int)W, (int)h, (int)w, (int)stride, img_blocks);
  } else {
    hipLaunchKernelGGL((ibp::augment_warp_kernel<float>), grid, block, 0, stream,
                       src, dp, img.data_ptr<float>(), miss.data_ptr<float>(),
                       all.data_ptr<float>(), (int)H, (int)W, (int)h, (int)w,
                       (int)stride, img_blocks);
  }
  IBP_CHECK_HIP(hipGetLastError());
  return {img, miss, all};
}
