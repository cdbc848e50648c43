// Limb scoring and device-side limb matching.
//
// limb_scores        candidate list in, [score, pass ratio, length] out; the
//                    host then filters and matches (find_connections_batch).
// peaks_canonical    the peak buffer of peaks_batched (arrival order) in the
//                    host's (channel, y, x) order, plus per-channel offsets.
// limb_match         per (image, limb type): enumerate nA x nB segments, score
//                    them, apply the two acceptance criteria and do the greedy
//                    1-1 matching; finished connection rows come out.
//
// The segment arithmetic lives in limb_segment_score(), shared by
// limb_score_kernel and limb_match_kernel so that both produce the same fp32
// values and the device matching ranks candidates exactly as the host does.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <climits>
#include "common.h"

namespace ibp {

struct LimbScore {
  float s_prior;     // mean PAF sample + distance prior
  float pass_ratio;  // share of samples above thre2
  float length;      // segment length (+1e-9)
};

// Sample min(round(len) + 1, mid_num) points along A->B on one limb plane
// (reference evaluate.py:228-240). Sample coordinates are clamped into the
// plane, so no peak coordinate can address outside it.
template <typename T>
__device__ __forceinline__ LimbScore limb_segment_score(
    const T* __restrict__ plane, float ax, float ay, float bx, float by,
    int H, int W, int mid_num, float thre2) {
  float dx = bx - ax, dy = by - ay;
  float len = sqrtf(dx * dx + dy * dy) + 1e-9f;
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
  LimbScore r;
  r.s_prior = mean + prior;
  r.pass_ratio = (float)pass / mn;
  r.length = len;
  return r;
}

// Score every candidate limb: emit [mean_score_with_dist_prior, pass_ratio,
// length]. grid: one thread per (limb_type, a, b) candidate triple (flattened).
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
    const LimbScore s = limb_segment_score(paf + (long long)limb * H * W,
                                           pa[1], pa[2], pb[1], pb[2], H, W,
                                           mid_num, thre2);
    scores[i * 3 + 0] = s.s_prior;
    scores[i * 3 + 1] = s.pass_ratio;
    scores[i * 3 + 2] = s.length;
  }
}

// ---- peaks_canonical ------------------------------------------------------

constexpr int kCanonMaxPeaks = 512;   // rows staged in LDS, ranked in O(P^2)
constexpr int kCanonThreads = 256;

// fp32 -> uint32 whose unsigned order is the float order (-0 counts as +0)
__device__ __forceinline__ unsigned int ordered_bits(float v) {
  const unsigned int u = __float_as_uint(v + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup per image. Rows of `buf` (block layout of peaks_batched: row 0
// = count as int32 bits, then rows in arrival order) are ranked by counting on
// the key (channel, refined y, refined x), ties by arrival slot, and written
// to peaks[n][rank]; a peak's id is its row index there. offsets[n][c] = rows
// of a channel < c, so channel c owns rows [offsets[c], offsets[c + 1]).
// Rows past the count are zeroed.
__global__ __launch_bounds__(kCanonThreads) void peaks_canonical_kernel(
    const float* __restrict__ buf, float* __restrict__ peaks,
    int* __restrict__ offsets, int C, int max_peaks) {
  __shared__ unsigned long long s_cy[kCanonMaxPeaks];   // channel << 32 | y
  __shared__ unsigned int s_x[kCanonMaxPeaks];
  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  const float* blk = buf + (long long)n * (1 + max_peaks) * 5;
  float* out = peaks + (long long)n * max_peaks * 5;
  // the counter keeps counting past the cap (atomicAdd precedes the cap test)
  const int cnt = min(max(__float_as_int(blk[0]), 0), max_peaks);

  for (int r = tid; r < cnt; r += kCanonThreads) {
    const float* row = blk + (long long)(1 + r) * 5;
    const float cf = row[0];              // clamped as a float: NaN -> 0
    const int c = cf >= (float)C ? C - 1 : (cf >= 0.f ? (int)cf : 0);
    s_cy[r] = ((unsigned long long)c << 32) | ordered_bits(row[2]);
    s_x[r] = ordered_bits(row[1]);
  }
  __syncthreads();

  for (int r = tid; r < cnt; r += kCanonThreads) {
    const unsigned long long cy = s_cy[r];
    const unsigned int x = s_x[r];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) {       // every lane reads slot j: broadcast
      const unsigned long long cyj = s_cy[j];
      const unsigned int xj = s_x[j];
      rank += (cyj < cy) || (cyj == cy && (xj < x || (xj == x && j < r)));
    }
    const float* row = blk + (long long)(1 + r) * 5;
    float* dst = out + (long long)rank * 5;   // rank < cnt <= max_peaks
    dst[0] = (float)(int)(cy >> 32);
    dst[1] = row[1]; dst[2] = row[2]; dst[3] = row[3]; dst[4] = row[4];
  }
  for (int i = cnt * 5 + tid; i < max_peaks * 5; i += kCanonThreads) out[i] = 0.f;

  for (int c = tid; c <= C; c += kCanonThreads) {
    int below = 0;
    for (int j = 0; j < cnt; ++j) below += (int)(s_cy[j] >> 32) < c;
    offsets[(long long)n * (C + 1) + c] = below;
  }
}

// ---- limb_match -----------------------------------------------------------

constexpr int kMatchMaxPart = 64;     // one 64-bit mask per side
constexpr int kMatchThreads = 256;
constexpr int kMatchWaves = kMatchThreads / kWave;
constexpr int kNoCand = INT_MAX;

// (key, idx) beats (bkey, bidx): larger key, then smaller index. kNoCand
// marks "nothing"; keys are never NaN (such candidates are not offered).
__device__ __forceinline__ bool cand_better(float key, int idx, float bkey,
                                            int bidx) {
  return idx != kNoCand && (bidx == kNoCand || key > bkey ||
                            (key == bkey && idx < bidx));
}

// One workgroup per (limb type, image). Candidate (i, j) sits at tile slot
// i * 64 + j, so slot order is the host's enumeration order i * nB + j.
// s_prior <= 0 marks a candidate that failed a criterion (criterion 2 is
// s_prior > 0, so no survivor is lost). `combined` is recomputed in every
// argmax round from s_prior and the two peak scores: (0.5 s + 0.25 a) + 0.25 b
// in fp32, the host's value; its products are exact, so contraction to FMA
// cannot change it.
//
// counts[n][k]: connections written, -1 if a part has no peak (special_k),
// -2 if a part has more than max_part peaks (the caller redoes that image).
// rows[n][k][r] = [idA, idB, s_prior, i, j, length].
__global__ __launch_bounds__(kMatchThreads) void limb_match_kernel(
    const float* __restrict__ maps,     // (N, planes, H, W)
    const float* __restrict__ peaks,    // (N, max_peaks, 5) canonical order
    const int* __restrict__ offsets,    // (N, C + 1)
    const int* __restrict__ limbs,      // (L, 2) part indices
    float* __restrict__ rows,           // (N, L, max_part, 6)
    int* __restrict__ counts,           // (N, L)
    int C, int L, int planes, int H, int W, int max_peaks,
    int first_limb_plane, int mid_num, float thre2, float connect_ration,
    int max_part) {
  __shared__ float s_prior[kMatchMaxPart * kMatchMaxPart];
  __shared__ float s_len[kMatchMaxPart * kMatchMaxPart];
  __shared__ float s_pa[3][kMatchMaxPart];   // x, y, score of the A peaks
  __shared__ float s_pb[3][kMatchMaxPart];
  __shared__ float s_wkey[kMatchWaves];
  __shared__ int s_widx[kMatchWaves];

  const int k = blockIdx.x, n = blockIdx.y;
  const int tid = threadIdx.x;
  int* count_out = counts + (long long)n * L + k;

  // every index read from memory is range-checked before it addresses memory
  const int a_part = limbs[k * 2 + 0], b_part = limbs[k * 2 + 1];
  int offA = 0, nA = 0, offB = 0, nB = 0;
  const int* off = offsets + (long long)n * (C + 1);
  if (a_part >= 0 && a_part < C) {
    offA = min(max(off[a_part], 0), max_peaks);
    nA = max(min(max(off[a_part + 1], 0), max_peaks) - offA, 0);
  }
  if (b_part >= 0 && b_part < C) {
    offB = min(max(off[b_part], 0), max_peaks);
    nB = max(min(max(off[b_part + 1], 0), max_peaks) - offB, 0);
  }
  if (nA == 0 || nB == 0) {             // uniform over the workgroup
    if (tid == 0) *count_out = -1;
    return;
  }
  if (nA > max_part || nB > max_part) {
    if (tid == 0) *count_out = -2;
    return;
  }

  const float* img_peaks = peaks + (long long)n * max_peaks * 5;
  if (tid < nA) {
    const float* p = img_peaks + (long long)(offA + tid) * 5;
    s_pa[0][tid] = p[1]; s_pa[1][tid] = p[2]; s_pa[2][tid] = p[3];
  } else if (tid >= kMatchMaxPart && tid - kMatchMaxPart < nB) {
    const int j = tid - kMatchMaxPart;
    const float* p = img_peaks + (long long)(offB + j) * 5;
    s_pb[0][j] = p[1]; s_pb[1][j] = p[2]; s_pb[2][j] = p[3];
  }
  __syncthreads();

  // score all nA x nB segments and apply the host's filters
  const float* plane =
      maps + ((long long)n * planes + first_limb_plane + k) * H * W;
  for (int c = tid; c < nA * nB; c += kMatchThreads) {
    const int i = c / nB, j = c - i * nB;
    const LimbScore s = limb_segment_score(plane, s_pa[0][i], s_pa[1][i],
                                           s_pb[0][j], s_pb[1][j], H, W,
                                           mid_num, thre2);
    // zero-length segments are rejected; criterion 1: enough samples above
    // thre2; criterion 2: positive score
    const bool keep = !(s.length < 1e-6f) && s.pass_ratio >= connect_ration &&
                      s.s_prior > 0.f;
    s_prior[i * kMatchMaxPart + j] = keep ? s.s_prior : -1.f;
    s_len[i * kMatchMaxPart + j] = s.length;
  }
  __syncthreads();

  // greedy 1-1 matching: per round the best unused (i, j), ties to the
  // smaller slot, which is what the host's stable sort over enumeration
  // order does
  unsigned long long usedA = 0ull, usedB = 0ull;
  const int rounds = min(nA, nB);
  float* out = rows + ((long long)n * L + k) * max_part * 6;
  int nconn = 0;
  while (nconn < rounds) {
    float bkey = 0.f;
    int bidx = kNoCand;
    for (int c = tid; c < nA * kMatchMaxPart; c += kMatchThreads) {
      const int i = c >> 6, j = c & 63;
      if (j >= nB || ((usedA >> i) & 1ull) || ((usedB >> j) & 1ull)) continue;
      const float s = s_prior[c];
      if (!(s > 0.f)) continue;
      const float key = (0.5f * s + 0.25f * s_pa[2][i]) + 0.25f * s_pb[2][j];
      // slots ascend within a thread, so a tie keeps the earlier one
      if (key == key && cand_better(key, c, bkey, bidx)) {
        bkey = key;
        bidx = c;
      }
    }
    #pragma unroll
    for (int m = 32; m > 0; m >>= 1) {   // butterfly: every lane ends equal
      const float okey = __shfl_xor(bkey, m, 64);
      const int oidx = __shfl_xor(bidx, m, 64);
      if (cand_better(okey, oidx, bkey, bidx)) {
        bkey = okey;
        bidx = oidx;
      }
    }
    if ((tid & 63) == 0) {
      s_wkey[tid >> 6] = bkey;
      s_widx[tid >> 6] = bidx;
    }
    __syncthreads();
    bkey = s_wkey[0];
    bidx = s_widx[0];
    #pragma unroll
    for (int w = 1; w < kMatchWaves; ++w) {
      const float okey = s_wkey[w];
      const int oidx = s_widx[w];
      if (cand_better(okey, oidx, bkey, bidx)) {
        bkey = okey;
        bidx = oidx;
      }
    }
    __syncthreads();                     // slots are rewritten next round
    if (bidx == kNoCand) break;          // uniform: all threads read the same
    const int i = bidx >> 6, j = bidx & 63;
    if (tid == 0) {
      float* r = out + nconn * 6;        // nconn < rounds <= max_part
      r[0] = (float)(offA + i);
      r[1] = (float)(offB + j);
      r[2] = s_prior[bidx];
      r[3] = (float)i;
      r[4] = (float)j;
      r[5] = s_len[bidx];
    }
    usedA |= 1ull << i;
    usedB |= 1ull << j;
    ++nconn;
  }
  if (tid == 0) *count_out = nconn;
}

}  // namespace ibp

using torch::Tensor;
static inline hipStream_t cur_stream_lm() {
  return at::hip::getCurrentHIPStream().stream();
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
                       cur_stream_lm(),
                       reinterpret_cast<const scalar_t*>(paf.data_ptr()),
                       peaks.data_ptr<float>(), cand_idx.data_ptr<int>(),
                       scores.data_ptr<float>(), ncand, H, W, (int)mid_num,
                       (float)thre2);
  });
  return scores;
}

// buf: fp32 (N, 1 + max_peaks, 5) as peaks_batched returns it. Returns
// {peaks fp32 (N, max_peaks, 5), offsets int32 (N, n_parts + 1)}.
std::vector<Tensor> peaks_canonical(const Tensor& buf, int64_t n_parts) {
  TORCH_CHECK(buf.is_cuda() && buf.dim() == 3 && buf.is_contiguous() &&
              buf.scalar_type() == at::kFloat && buf.size(2) == 5 &&
              buf.size(1) >= 2,
              "peaks_canonical: buf must be contiguous fp32 (N, 1 + max_peaks, 5)");
  const int N = (int)buf.size(0);
  const int max_peaks = (int)buf.size(1) - 1;
  TORCH_CHECK(max_peaks <= ibp::kCanonMaxPeaks, "peaks_canonical: max_peaks ",
              max_peaks, " exceeds the kernel's ", ibp::kCanonMaxPeaks);
  TORCH_CHECK(n_parts >= 1 && n_parts < (1 << 20), "peaks_canonical: bad n_parts");
  Tensor peaks = torch::empty({N, max_peaks, 5}, buf.options());
  Tensor offsets = torch::empty({N, n_parts + 1},
                                buf.options().dtype(torch::kInt32));
  if (N == 0) return {peaks, offsets};
  hipLaunchKernelGGL(ibp::peaks_canonical_kernel, dim3(N),
                     dim3(ibp::kCanonThreads), 0, cur_stream_lm(),
                     buf.data_ptr<float>(), peaks.data_ptr<float>(),
                     offsets.data_ptr<int>(), (int)n_parts, max_peaks);
  return {peaks, offsets};
}

// maps: planar fp32 (N, planes, H, W), limb planes from first_limb_plane;
// peaks / offsets as peaks_canonical returns them; limbs int32 (L, 2).
// Returns {rows fp32 (N, L, max_part, 6), counts int32 (N, L)}; only the
// first counts[n][k] rows of a limb are defined.
std::vector<Tensor> limb_match(const Tensor& maps, const Tensor& peaks,
                               const Tensor& offsets, const Tensor& limbs,
                               int64_t first_limb_plane, int64_t mid_num,
                               double thre2, double connect_ration,
                               int64_t max_part) {
  TORCH_CHECK(maps.is_cuda() && maps.dim() == 4 && maps.is_contiguous() &&
              maps.scalar_type() == at::kFloat,
              "limb_match: maps must be contiguous fp32 (N, planes, H, W)");
  const int N = (int)maps.size(0), planes = (int)maps.size(1);
  const int H = (int)maps.size(2), W = (int)maps.size(3);
  TORCH_CHECK(peaks.is_cuda() && peaks.dim() == 3 && peaks.is_contiguous() &&
              peaks.scalar_type() == at::kFloat && peaks.size(0) == N &&
              peaks.size(1) >= 1 && peaks.size(2) == 5,
              "limb_match: peaks must be contiguous fp32 (N, max_peaks, 5)");
  TORCH_CHECK(offsets.is_cuda() && offsets.dim() == 2 && offsets.is_contiguous() &&
              offsets.scalar_type() == at::kInt && offsets.size(0) == N &&
              offsets.size(1) >= 2,
              "limb_match: offsets must be contiguous int32 (N, n_parts + 1)");
  TORCH_CHECK(limbs.is_cuda() && limbs.dim() == 2 && limbs.is_contiguous() &&
              limbs.scalar_type() == at::kInt && limbs.size(1) == 2 &&
              limbs.size(0) >= 1,
              "limb_match: limbs must be contiguous int32 (L, 2)");
  const int L = (int)limbs.size(0), C = (int)offsets.size(1) - 1;
  TORCH_CHECK(H >= 1 && W >= 1 && N <= 65535, "limb_match: bad map shape");
  TORCH_CHECK(first_limb_plane >= 0 && first_limb_plane + L <= planes,
              "limb_match: limb planes [", first_limb_plane, ", ",
              first_limb_plane + L, ") outside the ", planes, " planes of maps");
  TORCH_CHECK(max_part >= 1 && max_part <= ibp::kMatchMaxPart,
              "limb_match: max_part must be in [1, ", ibp::kMatchMaxPart, "]");
  TORCH_CHECK(mid_num >= 1, "limb_match: bad mid_num");
  Tensor rows = torch::empty({N, L, max_part, 6}, maps.options());
  Tensor counts = torch::empty({N, L}, maps.options().dtype(torch::kInt32));
  if (N == 0) return {rows, counts};
  hipLaunchKernelGGL(ibp::limb_match_kernel, dim3(L, N),
                     dim3(ibp::kMatchThreads), 0, cur_stream_lm(),
                     maps.data_ptr<float>(), peaks.data_ptr<float>(),
                     offsets.data_ptr<int>(), limbs.data_ptr<int>(),
                     rows.data_ptr<float>(), counts.data_ptr<int>(), C, L,
                     planes, H, W, (int)peaks.size(1), (int)first_limb_plane,
                     (int)mid_num, (float)thre2, (float)connect_ration,
                     (int)max_part);
  return {rows, counts};
}
