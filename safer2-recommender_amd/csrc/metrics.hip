// metrics.hip -- Recall@K and NDCG@K of ranked lists that are still in device
// memory: the last step of frecsys_rank_metrics, run on rec_merge_kernel's
// out_items right after the fused scoring + top-K of a row batch
// (recommend.hip).  Restates frecsys_list_metrics (serve.hip; the reference's
// RankMetrics, recommender.h:152-182) operation for operation, so that the two
// agree bitwise:
//
//   rank_metrics_kernel  one wave per query row, four rows per workgroup.
//                        Lane l tests ranks l, l + 64, ... of the row's list
//                        against the row's ground truth (sorted, distinct ids:
//                        a binary search); __ballot makes one 64-bit hit word
//                        per 64 ranks, at most 16 of them, in every lane's
//                        registers.  Lane q < nk then owns cut-off k_list[q]:
//                        hits = the popcount of the first k_q bits, dcg = the
//                        sum of gain[j] over the set bits in ascending rank j
//                        (double), norm = idcg[min(k_q, g)].
//
// Why equality and not a tolerance: the host adds 1.0 per hit in double (exact,
// so the popcount converted to double is that sum), adds gain[j] =
// 1 / log2(j + 2) to a double dcg from 0.0 in ascending j (the kernel adds the
// host's own table entries in the same order), forms norm as the sequential
// prefix sum of the same table (the kernel reads the host's prefix), and
// divides in double before rounding to float.  Every device operation is an
// IEEE add, divide or convert on identical operands; the build has no
// fast-math flag, so the double division is the correctly rounded one.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;

constexpr int kRowsPerBlock = 4;
constexpr int kWords = kMetricMaxK / 64;  // hit words of one row

__global__ void __launch_bounds__(64 * kRowsPerBlock) rank_metrics_kernel(RankMetricsArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= a.n) return;  // the whole wave
  const int64_t g0 = a.gt_ptr[a.r0 + row], g1 = a.gt_ptr[a.r0 + row + 1];
  const int32_t* __restrict__ gt = a.gt;
  const int32_t* __restrict__ list = a.lists + row * a.k;
  u64 w[kWords];
#pragma unroll
  for (int t = 0; t < kWords; ++t) {
    w[t] = 0;
    if (t * 64 < a.k) {  // wave-uniform
      const int j = t * 64 + lane;
      bool hit = false;
      if (j < a.k) {
        const int32_t id = list[j];
        if (id >= 0) {  // -1: an empty slot
          int64_t lo = g0, hi = g1;
          while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (gt[mid] < id) lo = mid + 1;
            else hi = mid;
          }
          hit = lo < g1 && gt[lo] == id;
        }
      }
      w[t] = __ballot(hit);
    }
  }
  if (lane >= a.nk) return;
  const int kq = a.k_list[lane];  // 1 .. a.k
  const int64_t g = g1 - g0;      // distinct ground-truth ids, >= 1
  int hits = 0;
  double dcg = 0.0;
#pragma unroll
  for (int t = 0; t < kWords; ++t) {
    const int left = kq - t * 64;  // ranks of this word below the cut-off
    if (left > 0) {
      u64 b = left >= 64 ? w[t] : (w[t] & ((1ull << left) - 1ull));
      hits += __popcll(b);
      while (b) {
        dcg += a.gain[t * 64 + (__ffsll((long long)b) - 1)];
        b &= b - 1;
      }
    }
  }
  const double norm = a.idcg[(int64_t)kq < g ? (int64_t)kq : g];
  const float fk = (float)kq, fg = (float)g;
  const float mn = fk < fg ? fk : fg;  // std::min<float>((float)k, (float)g)
  a.recall[row * a.nk + lane] = (float)((double)hits / (double)mn);
  a.ndcg[row * a.nk + lane] = (float)(dcg / norm);
}

}  // namespace

hipError_t launch_rank_metrics(const RankMetricsArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.k < 1 || a.k > kMetricMaxK || a.nk < 1 || a.nk > kMetricMaxCutoffs || !a.lists ||
      !a.gt_ptr || !a.gt || !a.k_list || !a.gain || !a.idcg || !a.recall || !a.ndcg)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(rank_metrics_kernel,
                     dim3((unsigned)((a.n + kRowsPerBlock - 1) / kRowsPerBlock)),
                     dim3(64 * kRowsPerBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace frecsys_hip
