// On-device keypoint post-processing primitives.
//
// Replaces the reference's CPU-bound post-process stages (5.2 FPS headline
// bottleneck, reference README.md:68): peak NMS (utils/util.py:177-183),
// sub-pixel centroid refinement (:186-211) and the 20-point limb line-integral
// scoring of find_connections (evaluate.py:206-276). The tiny greedy assembly
// stays on the host, consuming the device-scored candidates.
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

// Score every candidate limb: sample mid_num points along each A->B segment on
// the limb channel; emit [mean_score_with_dist_prior, pass_ratio, length].
// grid: one thread per (limb_type, a, b) candidate triple (flattened).
template <typename T>
__global__ void limb_score_kernel(
    const T* __restrict__ paf,          // [Cpaf, H, W]
    const float* __restrict__ peaks,    // [P][5] rows as peaks_batched writes
    const int* __restrict__ cand_idx,   // [ncand][3]: limb_id, peakA, peakB
    float* __restrict__ scores,         // [ncand][3]
    int ncand, int H, int W, int mid_num, float thre2) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ncand;
       i += gridDim.x * blockDim.x) {
    int limb = cand_idx[i * 3 + 0];
    const float* pa = peaks + (long long)cand_idx[i * 3 + 1] * 5;
    const float* pb = peaks + (long long)cand_idx[i * 3 + 2] * 5;
    float ax = pa[1], ay = pa[2], bx = pb[1], by = pb[2];
    float dx = bx - ax, dy = by - ay;
    float len = sqrtf(dx * dx + dy * dy) + 1e-9f;
    const T* plane = paf + (long long)limb * H * W;
    float sum = 0.f;
    int pass = 0;
    // short limbs sample fewer points (reference evaluate.py:228:
    // mid_num = min(round(norm)+1, param mid_num))
    const int mn = min((int)roundf(len) + 1, mid_num);
    for (int k = 0; k < mn; ++k) {
      float t = mn == 1 ? 0.f : (float)k / (mn - 1);
      int x = (int)roundf(ax + t * dx);
      int y = (int)roundf(ay + t * dy);
      x = min(max(x, 0), W - 1);
      y = min(max(y, 0), H - 1);
      float v = ldf(plane + (long long)y * W + x);
      sum += v;
      if (v > thre2) ++pass;
    }
    float mean = sum / mn;
    // distance prior of the reference (evaluate.py:240): penalise limbs longer
    // than half the image height
    float prior = fminf(0.5f * H / len - 1.f, 0.f);
    scores[i * 3 + 0] = mean + prior;
    scores[i * 3 + 1] = (float)pass / mn;
    scores[i * 3 + 2] = len;
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

Tensor limb_scores(const Tensor& paf, const Tensor& peaks, const Tensor& cand_idx,
                   int64_t mid_num, double thre2) {
  int W = (int)paf.size(-1), H = (int)paf.size(-2);
  int ncand = (int)cand_idx.size(0);
  Tensor scores = torch::zeros({std::max(ncand, 1), 3},
                               paf.options().dtype(torch::kFloat32));
  if (ncand == 0) return scores;
  dim3 block(256), grid(ibp::grid_1d(ncand, 256, 2048));
  AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::BFloat16, at::ScalarType::Half,
      paf.scalar_type(), "limb_scores", [&] {
    hipLaunchKernelGGL(ibp::limb_score_kernel<scalar_t>, grid, block, 0,
                       cur_stream4(),
                       reinterpret_cast<const scalar_t*>(paf.data_ptr()),
                       peaks.data_ptr<float>(), cand_idx.data_ptr<int>(),
                       scores.data_ptr<float>(), ncand, H, W, (int)mid_num,
                       (float)thre2);
  });
  return scores;
}
