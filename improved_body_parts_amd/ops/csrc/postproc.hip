// On-device keypoint post-processing primitives.
//
// Replaces the reference's CPU-bound post-process stages (5.2 FPS headline
// bottleneck, reference README.md:68): peak NMS (utils/util.py:177-183) and
// sub-pixel centroid refinement (:186-211). The 20-point limb line-integral
// scoring of find_connections (evaluate.py:206-276) and the device-side
// matching are in limb_match.hip.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace ibp {

// Peaks: 3x3 max-pool-equality NMS with reflect border + threshold, and
// sub-pixel centroid refinement of every survivor, in one pass over the
// keypoint planes [n][0..C) of a planar (N, planes_per_image, H, W) fp32
// buffer. Counters and the max_peaks cap are per image. Image n's block of
// `out` is [1 + max_peaks][5]: row 0 holds the peak count (as int32 bits) so
// counts and rows come back in one device->host copy; rows
// [channel, x_refined, y_refined, score_box_mean, peak_score] follow in
// arrival order.
__global__ void peaks_batched_kernel(const float* __restrict__ maps,
                                     float* __restrict__ out,
                                     int N, int C, int planes_per_image,
                                     int H, int W, float thre, int radius,
                                     int max_peaks) {
  const long long per_img = (long long)C * H * W;
  const long long total = per_img * N;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i / per_img);
    long long q = i - (long long)n * per_img;
    const int w = (int)(q % W);
    q /= W;
    const int h = (int)(q % H);
    const int c = (int)(q / H);
    const float* plane = maps + ((long long)n * planes_per_image + c) * H * W;
    const float v = plane[(long long)h * W + w];
    if (!(v >= thre) || v <= 0.f) continue;
    float m = -1e30f;
    #pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      #pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        int hh = h + dy, ww = w + dx;
        hh = hh < 0 ? -hh : (hh >= H ? 2 * H - hh - 2 : hh);  // reflect
        ww = ww < 0 ? -ww : (ww >= W ? 2 * W - ww - 2 : ww);
        m = fmaxf(m, plane[(long long)hh * W + ww]);
      }
    }
    if (v != m) continue;
    float* blk = out + (long long)n * (1 + max_peaks) * 5;
    const int slot = atomicAdd(reinterpret_cast<int*>(blk), 1);
    if (slot >= max_peaks) continue;
    // weighted-centroid refinement over (2r+1)^2 (reference util.py:186-211)
    float xr = (float)w, yr = (float)h, boxmean = v;
    if (h - radius >= 0 && h + radius < H && w - radius >= 0 && w + radius < W) {
      float s = 0.f, sx = 0.f, sy = 0.f;
      for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
          float sv = plane[(long long)(h + dy) * W + (w + dx)];
          s += sv; sx += sv * dx; sy += sv * dy;
        }
      if (s > 0.f) {
        xr = w + sx / s;
        yr = h + sy / s;
        boxmean = s / ((2 * radius + 1) * (2 * radius + 1));
      }
    }
    float* row = blk + (long long)(1 + slot) * 5;
    row[0] = (float)c; row[1] = xr; row[2] = yr; row[3] = boxmean; row[4] = v;
  }
}

}  // namespace ibp

using torch::Tensor;
static inline hipStream_t cur_stream4() {
  return at::hip::getCurrentHIPStream().stream();
}

// maps: planar (N, planes, H, W) fp32; the first `heat_layers` planes of every
// image are searched. Returns fp32 (N, 1 + max_peaks, 5); see the kernel.
Tensor peaks_batched(const Tensor& maps, int64_t heat_layers, double thre,
                     int64_t radius, int64_t max_peaks) {
  TORCH_CHECK(maps.is_cuda() && maps.dim() == 4 && maps.is_contiguous() &&
              maps.scalar_type() == at::kFloat,
              "peaks_batched: maps must be contiguous fp32 (N, planes, H, W)");
  const int N = (int)maps.size(0), P = (int)maps.size(1);
  const int H = (int)maps.size(2), W = (int)maps.size(3);
  TORCH_CHECK(heat_layers >= 1 && heat_layers <= P, "peaks_batched: bad heat_layers");
  TORCH_CHECK(H >= 2 && W >= 2, "peaks_batched: reflect border needs H, W >= 2");
  TORCH_CHECK(max_peaks >= 1 && radius >= 0, "peaks_batched: bad max_peaks/radius");
  Tensor out = torch::zeros({N, 1 + max_peaks, 5}, maps.options());
  if (N == 0) return out;
  const long long total = (long long)N * heat_layers * H * W;
  dim3 block(256), grid(ibp::grid_1d(total, 256, 4096));
  hipLaunchKernelGGL(ibp::peaks_batched_kernel, grid, block, 0, cur_stream4(),
                     maps.data_ptr<float>(), out.data_ptr<float>(), N,
                     (int)heat_layers, P, H, W, (float)thre, (int)radius,
                     (int)max_peaks);
  return out;
}
