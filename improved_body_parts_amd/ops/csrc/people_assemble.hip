// Device-side person assembly: the greedy subset assembly of find_people
// (engine/inference.py, reference evaluate.py:279-498) over the connection rows
// limb_match leaves on the device, plus subsets_to_keypoints.
//
// One workgroup of one wave64 per image. The walk over limbs and, within a
// limb, over its connection rows in stored order is sequential and uniform
// over the wave; the 64 lanes share the scan over the live subset rows, and a
// 64-bit ballot per group of 64 rows gives the first two matches in table
// order. Every decision is taken from values all lanes read alike, so every
// branch is uniform; lane 0 (or lanes 0..17, one per part slot) writes.
//
// Bit-identical to the host: confidences, totals and lengths are fp64 widened
// from the same fp32 inputs, ids are integers, and every sum is written in the
// host's association. Contraction is off for this file, so no multiply is
// fused into a neighbouring add.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <climits>
#include <cmath>
#include "common.h"

#pragma clang fp contract(off)

namespace ibp {

constexpr int kAsmParts = 18;          // part slots of a subset row
constexpr int kAsmSlots = kAsmParts + 2;
constexpr int kAsmKeypoints = 17;      // COCO keypoints per person
constexpr int kAsmMaxPeople = 128;     // live subset rows held in LDS
constexpr int kAsmMaxPart = 64;        // a limb's rows sit one per lane
constexpr int kAsmMaxPeaks = 512;      // candidate scores staged in LDS
constexpr int kAsmIdStride = 19;       // odd: a column read has no bank conflict
constexpr int kAsmOverflow = -2;

// The subset table. A live row is named by its position in `live`; `live` is a
// permutation of the physical rows whose first n_live entries are the table in
// the host's order and whose tail is the free list.
struct AsmTable {
  double conf[kAsmMaxPeople * kAsmParts];   // slot confidence, -1 if empty
  double total[kAsmMaxPeople];              // host row -2, column 0
  double longest[kAsmMaxPeople];            // host row -1, column 1
  int id[kAsmMaxPeople * kAsmIdStride];     // slot candidate id, -1 if empty
  int count[kAsmMaxPeople];                 // host row -1, column 0
  int live[kAsmMaxPeople];
};

// Python's max(length, longest): the first argument unless the second is larger
__device__ __forceinline__ double asm_longest(double length, double longest) {
  return longest > length ? longest : length;
}

__global__ __launch_bounds__(kWave) void people_assemble_kernel(
    const float* __restrict__ peaks,     // (N, max_peaks, 5) canonical order
    const int* __restrict__ offsets,     // (N, kAsmParts + 1)
    const float* __restrict__ rows,      // (N, L, max_part, 6)
    const int* __restrict__ counts,      // (N, L)
    const int* __restrict__ limbs,       // (L, 2)
    const int* __restrict__ dt_gt,       // (kAsmParts): COCO slot of a part, -1 none
    int* __restrict__ n_people,          // (N)
    double* __restrict__ subset,         // (N, max_people, kAsmSlots, 2)
    float* __restrict__ keypoints,       // (N, max_people, kAsmKeypoints, 2)
    int L, int max_peaks, int max_part, int max_people, double len_rate,
    double connection_tole, int remove_recon) {
  __shared__ AsmTable t;
  __shared__ float s_score[kAsmMaxPeaks];

  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  const float* img_peaks = peaks + (long long)n * max_peaks * 5;
  const int* img_counts = counts + (long long)n * L;
  // ids are row indices below the image's peak count
  const int ncand =
      min(max(offsets[(long long)n * (kAsmParts + 1) + kAsmParts], 0), max_peaks);

  for (int r = lane; r < ncand; r += kWave) s_score[r] = img_peaks[r * 5 + 3];
  for (int q = lane; q < kAsmMaxPeople; q += kWave) t.live[q] = q;

  // an overflowed limb means the image has to be redone on the host
  bool bad = false;
  for (int k = lane; k < L; k += kWave) bad |= img_counts[k] < -1;
  if (__ballot(bad) != 0ull) {
    if (lane == 0) n_people[n] = kAsmOverflow;
    return;
  }
  __syncthreads();

  int n_live = 0;
  bool overflow = false;
  for (int k = 0; k < L && !overflow; ++k) {
    int cnt = img_counts[k];
    if (cnt < 0) continue;               // no peaks in a part: special_k
    cnt = min(cnt, max_part);
    const int ia = limbs[k * 2 + 0], ib = limbs[k * 2 + 1];
    if (ia < 0 || ia >= kAsmParts || ib < 0 || ib >= kAsmParts) {
      overflow = true;
      break;
    }
    // lane r holds connection row r of this limb
    float r_a = 0.f, r_b = 0.f, r_score = 0.f, r_len = 0.f;
    if (lane < cnt) {
      const float* row = rows + (((long long)n * L + k) * max_part + lane) * 6;
      r_a = row[0]; r_b = row[1]; r_score = row[2]; r_len = row[5];
    }
    for (int i = 0; i < cnt; ++i) {
      const float fa = __shfl(r_a, i, kWave), fb = __shfl(r_b, i, kWave);
      const double score = (double)__shfl(r_score, i, kWave);
      const double length = (double)__shfl(r_len, i, kWave);
      if (!(fa >= 0.f && fa < (float)ncand && fb >= 0.f && fb < (float)ncand)) {
        overflow = true;
        break;
      }
      const int pa = (int)fa, pb = (int)fb;

      // the first two live rows, in table order, holding A or B
      int found = 0, j1 = 0, j2 = 0;
      for (int base = 0; base < n_live && found < 2; base += kWave) {
        const int q = base + lane;
        bool hit = false;
        if (q < n_live) {
          const int r = t.live[q];
          hit = t.id[r * kAsmIdStride + ia] == pa ||
                t.id[r * kAsmIdStride + ib] == pb;
        }
        unsigned long long mask = __ballot(hit);
        while (mask != 0ull && found < 2) {
          const int pos = __ffsll(mask) - 1;
          if (found == 0) j1 = base + pos; else j2 = base + pos;
          ++found;
          mask &= mask - 1ull;
        }
      }

      if (found == 0) {
        // new person
        if (n_live >= max_people) {
          overflow = true;
          break;
        }
        const int r = t.live[n_live];
        if (lane < kAsmParts) {
          const bool set = lane == ia || lane == ib;
          t.id[r * kAsmIdStride + lane] = lane == ib ? pb : (lane == ia ? pa : -1);
          t.conf[r * kAsmParts + lane] = set ? score : -1.0;
        }
        if (lane == 0) {
          t.total[r] = ((double)s_score[pa] + (double)s_score[pb]) + score;
          t.count[r] = 2;
          t.longest[r] = length;
        }
        ++n_live;
      } else if (found == 1) {
        const int r = t.live[j1];
        const int id_b = t.id[r * kAsmIdStride + ib];
        const double conf_b = t.conf[r * kAsmParts + ib];
        const double longest = t.longest[r];
        if (id_b == -1 && len_rate * longest > length) {
          // B slot empty and the limb not absurdly long for this person
          if (lane == 0) {
            t.id[r * kAsmIdStride + ib] = pb;
            t.conf[r * kAsmParts + ib] = score;
            t.count[r] += 1;
            t.longest[r] = asm_longest(length, longest);
            t.total[r] += (double)s_score[pb] + score;
          }
        } else {
          bool replace;
          if (id_b != pb) {
            // overwrite unless the existing connection is more confident or
            // the limb is too long
            replace = !(conf_b >= score) && !(len_rate * longest <= length);
          } else {
            // the same keypoint again with a better score: refresh
            replace = conf_b <= score;
          }
          if (replace && lane == 0) {
            // an empty slot reads the last candidate, as numpy's [-1] does
            const int old = id_b < 0 ? ncand + id_b : id_b;
            double total = t.total[r];
            total -= (double)s_score[old] + conf_b;
            total += (double)s_score[pb] + score;
            t.total[r] = total;
            t.id[r * kAsmIdStride + ib] = pb;
            t.conf[r * kAsmParts + ib] = score;
            t.longest[r] = asm_longest(length, longest);
          }
        }
      } else {
        const int r1 = t.live[j1], r2 = t.live[j2];
        int id1 = -1, id2 = -1;
        double c1v = -1.0, c2v = -1.0;
        if (lane < kAsmParts) {
          id1 = t.id[r1 * kAsmIdStride + lane];
          id2 = t.id[r2 * kAsmIdStride + lane];
          c1v = t.conf[r1 * kAsmParts + lane];
          c2v = t.conf[r2 * kAsmParts + lane];
        }
        if (__ballot(id1 >= 0 && id2 >= 0) == 0ull) {
          // disjoint: merge if this limb is trustworthy
          double min1 = INFINITY, min2 = INFINITY;
          for (int s = 0; s < kAsmParts; ++s) {
            const double a = t.conf[r1 * kAsmParts + s];
            const double b = t.conf[r2 * kAsmParts + s];
            if (t.id[r1 * kAsmIdStride + s] >= 0 && a < min1) min1 = a;
            if (t.id[r2 * kAsmIdStride + s] >= 0 && b < min2) min2 = b;
          }
          const double min_tolerance = min2 < min1 ? min2 : min1;
          const double longest = t.longest[r1];
          const bool refused = score < connection_tole * min_tolerance ||
                               len_rate * longest <= length;
          if (!refused) {
            if (lane < kAsmParts) {
              // the host's arithmetic on both columns: x1 += x2 + 1
              t.id[r1 * kAsmIdStride + lane] = id1 + (id2 + 1);
              t.conf[r1 * kAsmParts + lane] = c1v + (c2v + 1.0);
            }
            // the shift below reads `live` before it writes
            int moved[kAsmMaxPeople / kWave];
            #pragma unroll
            for (int c = 0; c < kAsmMaxPeople / kWave; ++c) {
              const int q = j2 + 1 + c * kWave + lane;
              moved[c] = q < n_live ? t.live[q] : -1;
            }
            if (lane == 0) {
              double total = t.total[r1];
              total += t.total[r2];
              total += score;
              t.total[r1] = total;
              t.count[r1] += t.count[r2];
              t.longest[r1] = asm_longest(length, longest);
            }
            __syncthreads();
            // np.delete(subset, j2): later rows move up, r2 joins the free list
            #pragma unroll
            for (int c = 0; c < kAsmMaxPeople / kWave; ++c) {
              const int q = j2 + 1 + c * kWave + lane;
              if (q < n_live) t.live[q - 1] = moved[c];
            }
            if (lane == 0) t.live[n_live - 1] = r2;
            --n_live;
          }
        } else {
          // two people compete for this limb
          const unsigned long long a_in_1 = __ballot(lane < kAsmParts && id1 == pa);
          const unsigned long long b_in_1 = __ballot(lane < kAsmParts && id1 == pb);
          const unsigned long long a_in_2 = __ballot(lane < kAsmParts && id2 == pa);
          const unsigned long long b_in_2 = __ballot(lane < kAsmParts && id2 == pb);
          const unsigned long long m1 = a_in_1 != 0ull ? a_in_1 : b_in_1;
          const unsigned long long m2 = a_in_1 != 0ull ? b_in_2 : a_in_2;
          if (m1 != 0ull && m2 != 0ull) {
            const int c1 = __ffsll(m1) - 1, c2 = __ffsll(m2) - 1;
            const double conf1 = t.conf[r1 * kAsmParts + c1];
            const double conf2 = t.conf[r2 * kAsmParts + c2];
            const bool both_better = score < conf1 && score < conf2;
            if (!both_better && remove_recon > 0 && lane == 0) {
              const bool second = conf1 > conf2;
              const int rs = second ? r2 : r1, cs = second ? c2 : c1;
              const double conf_s = second ? conf2 : conf1;
              const int id_s = t.id[rs * kAsmIdStride + cs];   // pa or pb
              t.total[rs] -= (double)s_score[id_s] + conf_s;
              t.id[rs * kAsmIdStride + cs] = -1;
              t.conf[rs * kAsmParts + cs] = -1.0;
              t.count[rs] -= 1;
            }
          }
        }
      }
      __syncthreads();                   // lane 0's writes, before the next scan
    }
  }

  if (overflow) {                        // uniform
    if (lane == 0) n_people[n] = kAsmOverflow;
    return;
  }

  // the part whose coordinates fill COCO slot `lane`: the last one mapped to
  // it, as the host's loop over the mapping leaves it
  int my_part = -1;
  if (lane < kAsmKeypoints)
    for (int p = 0; p < kAsmParts; ++p)
      if (dt_gt[p] == lane) my_part = p;

  // prune (fewer than 2 parts, or mean score below 0.45) and write, in order
  int out = 0;
  for (int q = 0; q < n_live; ++q) {
    const int r = t.live[q];
    const int cnt = t.count[r];
    const double total = t.total[r];
    if (!(cnt >= 2 && total / (double)cnt >= 0.45)) continue;
    double* srow = subset + ((long long)n * max_people + out) * kAsmSlots * 2;
    if (lane < kAsmParts) {
      srow[lane * 2 + 0] = (double)t.id[r * kAsmIdStride + lane];
      srow[lane * 2 + 1] = t.conf[r * kAsmParts + lane];
    } else if (lane == kAsmParts) {
      srow[lane * 2 + 0] = total;
      srow[lane * 2 + 1] = -1.0;
    } else if (lane == kAsmParts + 1) {
      srow[lane * 2 + 0] = (double)cnt;
      srow[lane * 2 + 1] = t.longest[r];
    }
    if (lane < kAsmKeypoints) {
      const int id = my_part >= 0 ? t.id[r * kAsmIdStride + my_part] : -1;
      float* kp = keypoints +
          (((long long)n * max_people + out) * kAsmKeypoints + lane) * 2;
      kp[0] = id >= 0 ? img_peaks[id * 5 + 1] : 0.f;   // id < ncand <= max_peaks
      kp[1] = id >= 0 ? img_peaks[id * 5 + 2] : 0.f;
    }
    ++out;
  }
  if (lane == 0) n_people[n] = out;
}

}  // namespace ibp

using torch::Tensor;

// peaks / offsets as peaks_canonical returns them, rows / counts as limb_match
// does; limbs int32 (L, 2); dt_gt int32 (18): COCO slot per part, -1 for none.
// Returns {n_people int32 (N), subset fp64 (N, max_people, 20, 2), keypoints
// fp32 (N, max_people, 17, 2)}; rows [0, n_people[n]) of an image are defined,
// and n_people[n] = -2 marks an image the caller has to redo on the host.
std::vector<Tensor> people_assemble(const Tensor& peaks, const Tensor& offsets,
                                    const Tensor& rows, const Tensor& counts,
                                    const Tensor& limbs, const Tensor& dt_gt,
                                    double len_rate, double connection_tole,
                                    int64_t remove_recon, int64_t max_people) {
  TORCH_CHECK(peaks.is_cuda() && peaks.dim() == 3 && peaks.is_contiguous() &&
              peaks.scalar_type() == at::kFloat && peaks.size(2) == 5 &&
              peaks.size(1) >= 1 && peaks.size(1) <= ibp::kAsmMaxPeaks,
              "people_assemble: peaks must be contiguous fp32 (N, max_peaks <= ",
              ibp::kAsmMaxPeaks, ", 5)");
  const int64_t N = peaks.size(0);
  TORCH_CHECK(offsets.is_cuda() && offsets.dim() == 2 && offsets.is_contiguous() &&
              offsets.scalar_type() == at::kInt && offsets.size(0) == N &&
              offsets.size(1) == ibp::kAsmParts + 1,
              "people_assemble: offsets must be contiguous int32 (N, ",
              ibp::kAsmParts + 1, ")");
  TORCH_CHECK(rows.is_cuda() && rows.dim() == 4 && rows.is_contiguous() &&
              rows.scalar_type() == at::kFloat && rows.size(0) == N &&
              rows.size(1) >= 1 && rows.size(2) >= 1 &&
              rows.size(2) <= ibp::kAsmMaxPart && rows.size(3) == 6,
              "people_assemble: rows must be contiguous fp32 (N, L, max_part <= ",
              ibp::kAsmMaxPart, ", 6)");
  const int64_t L = rows.size(1);
  TORCH_CHECK(counts.is_cuda() && counts.dim() == 2 && counts.is_contiguous() &&
              counts.scalar_type() == at::kInt && counts.size(0) == N &&
              counts.size(1) == L,
              "people_assemble: counts must be contiguous int32 (N, L)");
  TORCH_CHECK(limbs.is_cuda() && limbs.dim() == 2 && limbs.is_contiguous() &&
              limbs.scalar_type() == at::kInt && limbs.size(0) == L &&
              limbs.size(1) == 2,
              "people_assemble: limbs must be contiguous int32 (L, 2)");
  TORCH_CHECK(dt_gt.is_cuda() && dt_gt.dim() == 1 && dt_gt.is_contiguous() &&
              dt_gt.scalar_type() == at::kInt && dt_gt.size(0) == ibp::kAsmParts,
              "people_assemble: dt_gt must be contiguous int32 (", ibp::kAsmParts,
              ")");
  TORCH_CHECK(max_people >= 1 && max_people <= ibp::kAsmMaxPeople,
              "people_assemble: max_people must be in [1, ", ibp::kAsmMaxPeople,
              "]");
  TORCH_CHECK(N <= INT_MAX && L <= (1 << 20), "people_assemble: batch too large");
  Tensor n_people = torch::empty({N}, peaks.options().dtype(torch::kInt32));
  Tensor subset = torch::empty({N, max_people, ibp::kAsmSlots, 2},
                               peaks.options().dtype(torch::kFloat64));
  Tensor keypoints = torch::empty({N, max_people, ibp::kAsmKeypoints, 2},
                                  peaks.options());
  if (N == 0) return {n_people, subset, keypoints};
  hipLaunchKernelGGL(ibp::people_assemble_kernel, dim3((unsigned)N),
                     dim3(ibp::kWave), 0,
                     at::hip::getCurrentHIPStream().stream(),
                     peaks.data_ptr<float>(), offsets.data_ptr<int>(),
                     rows.data_ptr<float>(), counts.data_ptr<int>(),
                     limbs.data_ptr<int>(), dt_gt.data_ptr<int>(),
                     n_people.data_ptr<int>(), subset.data_ptr<double>(),
                     keypoints.data_ptr<float>(), (int)L, (int)peaks.size(1),
                     (int)rows.size(2), (int)max_people, len_rate,
                     connection_tole, (int)remove_recon);
  return {n_people, subset, keypoints};
}
