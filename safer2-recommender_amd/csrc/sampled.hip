// sampled.hip -- the candidate lists of sampled evaluation, built on gfx950
// where rank_cand_kernel (rerank.hip) reads them: the kernels behind
// frecsys_sampled_metrics.  List of query row i = the row's distinct ground
// truth, then its negatives (include/frecsys_hip.h states the generator).
//
//   sampled_block_kernel  the row's "blocked" bits: bit j of bitmap[row] = 1
//                         for every j of the row's CSR history (with the
//                         exclude flag; rerank_history_kernel restated, that
//                         file keeps its kernel local) and of its ground truth;
//   sampled_pool_kernel   E = popcount(maskbits & ~blocked) over the row's
//                         words: the size of the pool the negatives come from;
//   sampled_fill_kernel   one wave per row.  Copies the ground truth to the
//                         head of the list.  A whole-pool row (2 n_neg > E or
//                         64 E < M) compacts maskbits & ~blocked to ids: lane
//                         l owns word w0 + l, a wave prefix sum of the
//                         popcounts places its ids, ascending.  A sampled row
//                         draws in blocks of 64: lane l computes draw t0 + l,
//                         tests its bit (blocked or already taken), drops a
//                         repeat of a lower lane (63 readlane compares), a
//                         64-bit ballot ranks the survivors, the first
//                         n_neg - have of them write their id at have + rank
//                         and set their bit.  Acceptance goes by lane order
//                         inside a block and the blocks run in order, so the
//                         result is the sequential definition's, draw for draw.
//
// The bits a block of draws sets are read by the next block of the same wave:
// they are set with a returning agent-scope atomic OR (complete in L2 before
// the wave goes on) and read with agent-scope atomic loads (served by L2, never
// by a stale L1 line).  The returned word also proves the invariant "an
// accepted id was not taken": a set bit there raises the fail word.
//
// No loop is unbounded: a sampled row has E >= 2 n_neg and 64 E >= M, so a
// draw is accepted with probability >= 1/128 while negatives are missing, and
// the loop stops at kSampleCapBase + kSampleCapPerNeg n_neg draws whatever
// happens, raising the fail word (frecsys_sample_negatives has the same cap).
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;

__global__ void __launch_bounds__(64) sampled_block_kernel(SampledArgs a) {
  const int64_t u = blockIdx.x, i = a.r0 + u;
  uint32_t* __restrict__ bm = a.bitmap + u * a.W;
  if (a.row_ptr) {
    const int64_t e = a.qrows ? a.qrows[i] : i;
    const int64_t p0 = a.row_ptr[e], p1 = a.row_ptr[e + 1];
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 64) {
      const int64_t j = a.col[p];
      if (j >= 0 && j < a.m) atomicOr(&bm[j >> 5], 1u << (j & 31));
    }
  }
  const int64_t g0 = a.gt_ptr[i], g1 = a.gt_ptr[i + 1];
  for (int64_t p = g0 + threadIdx.x; p < g1; p += 64) {
    const int64_t j = a.gt[p];
    if (j >= 0 && j < a.m) atomicOr(&bm[j >> 5], 1u << (j & 31));
  }
}

__global__ void __launch_bounds__(256) sampled_pool_kernel(SampledArgs a) {
  __shared__ int part[4];
  const int64_t u = blockIdx.x;
  const uint32_t* __restrict__ bm = a.bitmap + u * a.W;
  int c = 0;
  for (int64_t w = threadIdx.x; w < a.W; w += 256) c += __popc(a.maskw[w] & ~bm[w]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) a.pool[a.r0 + u] = part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(64) sampled_fill_kernel(SampledArgs a) {
  const int lane = threadIdx.x;
  const int64_t u = blockIdx.x, i = a.r0 + u;
  const int64_t g0 = a.gt_ptr[i], g = a.gt_ptr[i + 1] - g0;
  const int64_t p0 = a.cand_ptr[i] - a.cand_base;
  const int64_t room = a.cand_ptr[i + 1] - a.cand_base - p0 - g;  // slots behind the ground truth
  int32_t* __restrict__ list = a.cand + p0;
  for (int64_t p = lane; p < g; p += 64) list[p] = a.gt[g0 + p];
  int32_t* __restrict__ neg = list + g;
  uint32_t* bm = a.bitmap + u * a.W;
  const int64_t E = a.pool[i], n_neg = a.n_neg;
  if (2 * n_neg > E || 64 * E < a.M) {  // whole pool: every eligible id, ascending
    int64_t have = 0;
    for (int64_t w0 = 0; w0 < a.W; w0 += 64) {
      const int64_t w = w0 + lane;
      uint32_t bits = w < a.W ? a.maskw[w] & ~bm[w] : 0u;
      const int c = __popc(bits);
      int incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
      }
      int64_t pos = have + incl - c;
      while (bits) {
        const int b = __ffs((int)bits) - 1;
        if (pos < room) neg[pos] = (int32_t)(w * 32 + b);
        ++pos;
        bits &= bits - 1;
      }
      have += __shfl(incl, 63);
    }
    if (have != room && lane == 0) atomicMin(a.fail, (u64)i + 1);  // the count moved: never
    return;
  }
  if (room != n_neg) {  // the host sized the list by another rule: never
    if (lane == 0) atomicMin(a.fail, (u64)i + 1);
    return;
  }
  const int64_t r = a.qrows ? a.qrows[i] : i;
  const u64 key = mix64(a.seed + kGolden * (u64)(r + 1));
  const u64 cap = kSampleCapBase + kSampleCapPerNeg * (u64)n_neg;  // a multiple of 64
  const u64 below = (1ull << lane) - 1ull;
  int64_t have = 0;
  uint32_t broken = 0;
  for (u64 t0 = 0; have < n_neg; t0 += 64) {
    if (t0 >= cap) {
      broken = 1;
      break;
    }
    const u64 x = mix64(key + kGolden * (t0 + (u64)lane + 1ull));
    const u64 idx = ((x >> 32) * (u64)a.M) >> 32;  // < M
    const uint32_t j = a.dlist ? (uint32_t)a.dlist[idx] : (uint32_t)idx;
    const uint32_t bit = 1u << (j & 31);
    const uint32_t word = __hip_atomic_load(&bm[j >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool ok = !(word & bit);
#pragma unroll
    for (int s = 0; s < 63; ++s) {  // a repeat of a lower lane's draw
      const uint32_t js = (uint32_t)__builtin_amdgcn_readlane((int)j, s);
      if (s < lane && js == j) ok = false;
    }
    const u64 bal = __ballot(ok);
    const int rank = __popcll(bal & below);
    const int64_t need = n_neg - have;
    if (ok && rank < need) {
      neg[have + rank] = (int32_t)j;
      const uint32_t old =
          __hip_atomic_fetch_or(&bm[j >> 5], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      broken |= old & bit;
    }
    const int got = __popcll(bal);
    have += got < need ? got : need;
  }
  if (broken) atomicMin(a.fail, (u64)i + 1);
}

}  // namespace

hipError_t launch_sampled_pool(const SampledArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.m < 1 || a.W != recommend_words(a.m) || !a.maskw || !a.bitmap || !a.pool || !a.gt_ptr ||
      !a.gt || (a.row_ptr && !a.col))
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.bitmap, 0, sizeof(uint32_t) * (size_t)a.n * (size_t)a.W, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sampled_block_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a);
  hipLaunchKernelGGL(sampled_pool_kernel, dim3((unsigned)a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sampled_fill(const SampledArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.m < 1 || a.W != recommend_words(a.m) || a.M < 0 || a.M > a.m || (a.M > 0 && a.M < a.m && !a.dlist) ||
      a.n_neg < 0 || !a.maskw || !a.bitmap || !a.pool || !a.gt_ptr || !a.gt || !a.cand_ptr ||
      !a.cand || !a.fail)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sampled_fill_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace frecsys_hip
