// dpp.hip -- greedy MAP of a determinantal point process over a pool of items
// per query row (frecsys_recommend_dpp, frecsys_diversify_dpp): the
// incremental Cholesky of Chen, Zhang and Zhou (NeurIPS 2018) in fp32.  The
// pool, the relevance and the similarity are diversify.hip's, and the pool
// Gramian is div_gram_kernel's, unchanged; the semantics are
// include/frecsys_hip.h's, to the bit; frecsys_dpp_select (serve.hip) is the
// same in scalar C++.
//
//   dpp_select_kernel  one workgroup of W waves per row: W = 1 up to 256
//                      slots, 2 up to 512, 4 up to 1024.  Thread i owns the
//                      slots i, i + 64 W, ... (NS <= 4 of them) with the
//                      quality w, the residual r and the inverse norm in
//                      registers, the alive bits in one word.  A step forms
//                      the words score_key(w r + 0) << 32 | ~slot of the
//                      alive slots with r >= eps (key 0 for the alive slots
//                      below eps), takes their maximum over the wave (64-bit
//                      butterfly) and, for W > 1, over the waves (one LDS
//                      word per wave, double-buffered by the step's parity:
//                      one barrier per step); the residual of the wave's
//                      best slot travels with its word.  Thread 0 writes the
//                      outputs.  A zero key is the fallback: the word's low
//                      half is the lowest alive slot, and nothing else
//                      changes.  Otherwise the step reads row s of G
//                      (coalesced) and folds the rows 0 .. m-1 of the factor
//                      C ([step][pool] fp32) into NS chains per thread -- its
//                      own slots' columns times the broadcast value C[u][s],
//                      u ascending from +0, the loads of eight rows issued
//                      ahead of their fmas -- and writes row m of C
//                      (coalesced) and the new residuals.  C lies in LDS
//                      (FLDS) when 4 k pool bytes are at most kDppLdsBytes,
//                      else in the workspace of the call; the operations and
//                      their order are the same, so the bytes are.
//
// Nothing here depends on the batch, the grid or the other rows: a row's
// outputs are a function of its pool, the item table, theta, eps and the mode.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;

constexpr int kAhead = 8;  // rows of C whose loads are in flight together

__device__ __forceinline__ float inv_norm(float n2) {
  return n2 > 0.0f ? 1.0f / sqrtf(n2) : 0.0f;
}

template <int NS, int W, bool FLDS>
__global__ void __launch_bounds__(64 * W) dpp_select_kernel(DppArgs a) {
  // every multiply, subtraction, division and addition below is an operation
  // of its own (see the note in div_select_kernel); an fma is written as one
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float dpp_lds[];  // FLDS: C, [k][pool]
  __shared__ u64 x_best[2][W];
  __shared__ float x_rs[2][W];
  __shared__ float x_max[W], x_min[W];
  __shared__ int x_p[W];
  constexpr int T = 64 * W;  // threads of a row
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row = blockIdx.x;
  const int P = a.pool, k = a.k;
  const int32_t* ids = a.ids + row * P;
  const float* sc = a.pool_scores + row * P;
  const float* G = a.G + (size_t)row * P * P;
  float* C = FLDS ? dpp_lds : a.C + (size_t)row * k * P;
  int32_t* items = a.out_items + row * k;
  float* scores = a.out_scores + row * k;
  float* gain = a.out_gain ? a.out_gain + row * k : nullptr;

  float w[NS], r[NS], inv[NS];
  int col[NS];  // the slot, or 0 beyond the pool: loads need no guard
  uint32_t alive = 0;
  float smax = -INFINITY, smin = INFINITY;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int b = tid + T * j;
    col[j] = b < P ? b : 0;
    w[j] = 0.0f;
    r[j] = 0.0f;
    inv[j] = 0.0f;
    if (b < P && ids[b] >= 0) {
      alive |= 1u << j;
      w[j] = sc[b];
      const float n2 = G[(size_t)b * P + b];
      inv[j] = inv_norm(n2);
      r[j] = n2 > 0.0f ? 1.0f : 0.0f;
      smax = fmaxf(smax, w[j]);
      smin = fminf(smin, w[j]);
    }
  }
  int p = __popc(alive);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    smax = fmaxf(smax, __shfl_xor(smax, o, 64));
    smin = fminf(smin, __shfl_xor(smin, o, 64));
    p += __shfl_xor(p, o, 64);
  }
  if constexpr (W > 1) {
    if (lane == 0) {
      x_max[wave] = smax;
      x_min[wave] = smin;
      x_p[wave] = p;
    }
    __syncthreads();
    p = 0;
#pragma unroll
    for (int v = 0; v < W; ++v) {
      smax = fmaxf(smax, x_max[v]);
      smin = fminf(smin, x_min[v]);
      p += x_p[v];
    }
  }
  const float range = smax - smin;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    float rel = w[j];
    if (!a.raw) rel = range > 0.0f ? (w[j] - smin) / range : 0.0f;
    const float x = a.theta * rel;
    w[j] = dpp_exp2(fminf(fmaxf(x, -64.0f), 64.0f));
  }

  const float eps = a.eps;
  const int steps = p < k ? p : k;
  int m = 0;  // rows of C = DPP steps so far
  for (int t = 0; t < steps; ++t) {
    u64 best = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if ((alive >> j) & 1u) {
        const float v = w[j] * r[j] + 0.0f;
        const uint32_t key = r[j] >= eps ? score_key(v) : 0u;
        const u64 word = ((u64)key << 32) | (0xFFFFFFFFu - (uint32_t)(tid + T * j));
        best = word > best ? word : best;
      }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u64 x = __shfl_xor(best, o, 64);
      best = x > best ? x : best;
    }
    // the residual of the wave's best slot (a wave without an alive slot:
    // best = 0, no j matches, the value is never used)
    const uint32_t sw = 0xFFFFFFFFu - (uint32_t)best;
    float rs = 0.0f;
#pragma unroll
    for (int j = 0; j < NS; ++j) rs = sw / (uint32_t)T == (uint32_t)j ? r[j] : rs;
    rs = __shfl(rs, (int)(sw & 63u), 64);
    if constexpr (W > 1) {
      const int par = t & 1;
      if (lane == 0) {
        x_best[par][wave] = best;
        x_rs[par][wave] = rs;
      }
      __syncthreads();
#pragma unroll
      for (int v = 0; v < W; ++v) {
        const u64 x = x_best[par][v];
        if (x > best) {
          best = x;
          rs = x_rs[par][v];
        }
      }
    }
    const int s = (int)(0xFFFFFFFFu - (uint32_t)best);  // < P: some slot is alive
    const uint32_t key = (uint32_t)(best >> 32);
    if (tid == 0) {
      items[t] = ids[s];
      scores[t] = sc[s];
      if (gain) gain[t] = key ? score_unkey(key) : 0.0f;
    }
    if (s % T == tid) alive &= ~(1u << (s / T));
    // the fallback changes nothing; the last step's update is never read
    // (both conditions are the same in every thread of the row)
    if (key == 0u || t + 1 == steps) continue;

    const float delta = sqrtf(rs);
    const float* gs = G + (size_t)s * P;
    const float inv_s = inv_norm(gs[s]);
    float acc[NS], sim[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      acc[j] = 0.0f;
      sim[j] = (gs[col[j]] * inv_s) * inv[j] + 0.0f;
    }
    // (a column of a selected or empty slot holds stale or unwritten words:
    // read with the others, never used)
    int u = 0;
    for (; u + kAhead <= m; u += kAhead) {
      float cs[kAhead], cb[kAhead][NS];
#pragma unroll
      for (int q = 0; q < kAhead; ++q) {
        const float* cu = C + (size_t)(u + q) * P;
        cs[q] = cu[s];
#pragma unroll
        for (int j = 0; j < NS; ++j) cb[q][j] = cu[col[j]];
      }
#pragma unroll
      for (int q = 0; q < kAhead; ++q)
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] = __builtin_fmaf(cb[q][j], cs[q], acc[j]);
    }
    for (; u < m; ++u) {
      const float* cu = C + (size_t)u * P;
      const float cs = cu[s];
#pragma unroll
      for (int j = 0; j < NS; ++j) acc[j] = __builtin_fmaf(cu[col[j]], cs, acc[j]);
    }
    float* cm = C + (size_t)m * P;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if ((alive >> j) & 1u) {
        const float e = (sim[j] - acc[j]) / delta;
        cm[col[j]] = e;
        r[j] = __builtin_fmaf(-e, e, r[j]);
      }
    }
    ++m;
    // row m of C (LDS or global) is complete and visible to every thread of
    // the row: they read each other's columns
    __syncthreads();
  }
  for (int t = steps + tid; t < k; t += T) {
    items[t] = -1;
    scores[t] = -FLT_MAX;
    if (gain) gain[t] = -FLT_MAX;
  }
}

template <bool FLDS>
void launch_select(const DppArgs& a, size_t lds, hipStream_t s) {
  const dim3 grid((unsigned)a.n);
  if (a.pool <= 64)
    hipLaunchKernelGGL((dpp_select_kernel<1, 1, FLDS>), grid, dim3(64), lds, s, a);
  else if (a.pool <= 128)
    hipLaunchKernelGGL((dpp_select_kernel<2, 1, FLDS>), grid, dim3(64), lds, s, a);
  else if (a.pool <= 256)
    hipLaunchKernelGGL((dpp_select_kernel<4, 1, FLDS>), grid, dim3(64), lds, s, a);
  else if (a.pool <= 512)
    hipLaunchKernelGGL((dpp_select_kernel<4, 2, FLDS>), grid, dim3(128), lds, s, a);
  else
    hipLaunchKernelGGL((dpp_select_kernel<4, 4, FLDS>), grid, dim3(256), lds, s, a);
}

}  // namespace

size_t dpp_factor_bytes(int pool, int k) { return (size_t)4 * (size_t)k * (size_t)pool; }

bool dpp_factor_in_lds(int pool, int k) { return dpp_factor_bytes(pool, k) <= (size_t)kDppLdsBytes; }

hipError_t launch_dpp_select(const DppArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.pool < 1 || a.pool > kDiversifyMaxPool || a.k < 1 || a.k > a.pool || !a.ids ||
      !a.pool_scores || !a.G || !a.out_items || !a.out_scores || a.n > (int64_t)0x7fffffff)
    return hipErrorInvalidValue;
  if (!a.C) {
    if (!dpp_factor_in_lds(a.pool, a.k)) return hipErrorInvalidValue;
    launch_select<true>(a, dpp_factor_bytes(a.pool, a.k), s);
  } else {
    launch_select<false>(a, 0, s);
  }
  return hipGetLastError();
}

}  // namespace frecsys_hip
