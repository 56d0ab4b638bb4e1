// diversify.hip -- greedy maximal-marginal-relevance (MMR) re-ranking of a
// pool of items per query row (frecsys_recommend_diverse, frecsys_diversify).
// A row has `pool` slots of (item id, fp32 score); a negative id is an empty
// slot, ids may repeat (every slot is a candidate of its own).  The semantics
// are include/frecsys_hip.h's, to the bit; frecsys_mmr_select (serve.hip) is
// the same in scalar C++.
//
//   div_gram_kernel    G = T T^T per row, T = the item rows of the pool's
//                      slots (an empty slot: a zero row), on
//                      v_mfma_f32_32x32x2_f32 with the operands straight from
//                      the item table.  One wave per 64 x 64 block of the lower
//                      triangle (2 x 2 tiles: four loads of 16 B feed eight
//                      MFMAs), the blocks of a row dealt to the waves of its
//                      workgroups.  Lane (lo, hi) loads columns k0 .. k0 + 3 of
//                      its slot's row and supplies column k0 + hi, then
//                      k0 + 2 + hi: ONE accumulator chain per element over the
//                      whole padded dim in ascending k from +0, recommend.hip's
//                      and similar.hip's chain.  The products commute, so
//                      element (r, c) and element (c, r) are the same bits: a
//                      block below the diagonal is written twice, the mirror
//                      through a 32 x 33 LDS transpose of the wave's own so
//                      that both writes are coalesced.  The diagonal of G is
//                      n2 of the slots.
//   div_select_kernel  one wave per row; lane l owns the slots l, l + 64, ...
//                      (NS <= 16 of them) with base = lam * rel, the running
//                      maximum cosine m, the inverse norm and the alive bit in
//                      registers.  A step forms the words score_key(v) << 32 |
//                      ~slot of the alive slots, takes their maximum over the
//                      wave (64-bit butterfly), lets lane 0 write the outputs,
//                      then reads row s of G (coalesced) and folds
//                      (G[s][b] * inv_s) * inv_b + 0.0f into m.
//
// Nothing here depends on the batch, the grid or the other rows: a row's
// outputs are a function of its pool, the item table, lam and the mode alone.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;

constexpr int kGramWaves = 4;

// sqrtf and the division are correctly rounded in device code at hipcc's
// defaults (-fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn is not (it
// is the native square root, within 1 ulp).
__device__ __forceinline__ float inv_norm(float n2) {
  return n2 > 0.0f ? 1.0f / sqrtf(n2) : 0.0f;
}

__global__ void __launch_bounds__(64 * kGramWaves) div_gram_kernel(DiversifyArgs a, int groups) {
  __shared__ float tr[kGramWaves][32 * 33];
  const int lane = threadIdx.x & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int P = a.pool, Dp = a.Dp;
  const int TB = (P + 63) >> 6, NB = TB * (TB + 1) / 2;
  const int64_t row = blockIdx.x / groups;
  const int blk = (int)(blockIdx.x % groups) * kGramWaves + wave;
  if (row >= a.n || blk >= NB) return;  // wave-uniform; no workgroup barrier below
  int BI = 0;
  while ((BI + 1) * (BI + 2) / 2 <= blk) ++BI;
  const int BJ = blk - BI * (BI + 1) / 2;
  const int32_t* ids = a.ids + row * P;
  float* G = a.G + (size_t)row * P * P;

  // the lane's four slots: rows 64 BI + 32 u + lo (A) and 64 BJ + 32 u + lo (B)
  const float* pa[2];
  const float* pb[2];
  bool la[2], lb[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int sa = 64 * BI + 32 * u + lo, sb = 64 * BJ + 32 * u + lo;
    const int ia = sa < P ? ids[sa] : -1, ib = sb < P ? ids[sb] : -1;
    la[u] = ia >= 0;
    lb[u] = ib >= 0;
    pa[u] = a.Y + (int64_t)(la[u] ? ia : 0) * Dp;
    pb[u] = a.Y + (int64_t)(lb[u] ? ib : 0) * Dp;
  }
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  auto ld = [](const float* p, bool live, int k0) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) v = *reinterpret_cast<const float4*>(p + k0);
    return v;
  };
  // (values, not lvalues: a conditional on two members is a selected address)
  auto pick = [](bool second, float x, float y) { return second ? y : x; };
  f32x16 acc[2][2] = {{f32x16{0.f}, f32x16{0.f}}, {f32x16{0.f}, f32x16{0.f}}};
  float4 va[2] = {ld(pa[0], la[0], 0), ld(pa[1], la[1], 0)};
  float4 vb[2] = {ld(pb[0], lb[0], 0), ld(pb[1], lb[1], 0)};
#pragma unroll 1
  for (int k0 = 0; k0 < Dp; k0 += 4) {
    // the next step's rows are on their way during this step's MFMAs
    float4 na[2] = {zero, zero}, nb[2] = {zero, zero};
    if (k0 + 4 < Dp) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        na[u] = ld(pa[u], la[u], k0 + 4);
        nb[u] = ld(pb[u], lb[u], k0 + 4);
      }
    }
    float a0[2], a1[2], b0[2], b1[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      a0[u] = pick(hi, va[u].x, va[u].y);
      a1[u] = pick(hi, va[u].z, va[u].w);
      b0[u] = pick(hi, vb[u].x, vb[u].y);
      b1[u] = pick(hi, vb[u].z, vb[u].w);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = mfma32(a0[u], b0[v], acc[u][v]);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = mfma32(a1[u], b1[v], acc[u][v]);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      va[u] = na[u];
      vb[u] = nb[u];
    }
  }

  float* t = tr[wave];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int r0 = 64 * BI + 32 * u, c0 = 64 * BJ + 32 * v;
      if (r0 >= P || c0 >= P) continue;  // wave-uniform
      // element (r0 + acc_row(q, hi), c0 + lo)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = r0 + acc_row(q, hi), c = c0 + lo;
        if (r < P && c < P) G[(size_t)r * P + c] = acc[u][v][q];
      }
      if (BI == BJ) continue;  // the diagonal block holds both halves itself
#pragma unroll
      for (int q = 0; q < 16; ++q) t[acc_row(q, hi) * 33 + lo] = acc[u][v][q];
      wave_lds_sync();
      // element (c0 + acc_row(q, hi), r0 + lo) = its mirror's bits
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = c0 + acc_row(q, hi), r = r0 + lo;
        if (r < P && c < P) G[(size_t)c * P + r] = t[lo * 33 + acc_row(q, hi)];
      }
      wave_lds_sync();
    }
}

// The chain of a Gramian element in scalar code: acc = fma(x[c], y[c], acc), c
// ascending from +0 over the padded dim -- the MFMA's bits (similar.hip's
// norms and rerank.hip's scores rely on the same identity).
__device__ __forceinline__ float row_dot(const float* x, const float* y, int Dp) {
  float acc = 0.0f;
  for (int c = 0; c < Dp; c += 4) {
    const float4 u = *reinterpret_cast<const float4*>(x + c);
    const float4 v = *reinterpret_cast<const float4*>(y + c);
    acc = __builtin_fmaf(u.x, v.x, acc);
    acc = __builtin_fmaf(u.y, v.y, acc);
    acc = __builtin_fmaf(u.z, v.z, acc);
    acc = __builtin_fmaf(u.w, v.w, acc);
  }
  return acc;
}

// LAZY: no Gramian -- row s_t of it is computed each step from the item table
// (NS chains per lane side by side, the selected row read by every lane), and
// the norms at the start.  The same bits, k pool d products instead of
// pool^2 d / 2, no workspace.
template <int NS, bool LAZY>
__global__ void __launch_bounds__(256) div_select_kernel(DiversifyArgs a) {
  // Every multiply, subtraction and addition below is an operation of its
  // own: plain operators with contraction off.  (__fmul_rn / __fsub_rn are
  // plain operators defined under the header's contraction mode, so a pair of
  // them fuses into one fma at hipcc's default -ffp-contract.)
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n) return;  // wave-uniform
  const int P = a.pool, k = a.k;
  const int32_t* ids = a.ids + row * P;
  const float* sc = a.pool_scores + row * P;
  const float* G = LAZY ? nullptr : a.G + (size_t)row * P * P;
  const int Dp = a.Dp;
  int32_t* items = a.out_items + row * k;
  float* scores = a.out_scores + row * k;
  float* mmr = a.out_mmr ? a.out_mmr + row * k : nullptr;

  float base[NS], mm[NS], inv[NS];
  const float* yb[NS];  // LAZY: the slot's item row (row 0 for an empty slot: never used)
  uint32_t alive = 0;
  float smax = -INFINITY, smin = INFINITY;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int b = lane + 64 * j;
    base[j] = 0.0f;
    inv[j] = 0.0f;
    mm[j] = -INFINITY;
    yb[j] = a.Y;
    if (b < P && ids[b] >= 0) {
      alive |= 1u << j;
      base[j] = sc[b];
      if constexpr (LAZY) {
        yb[j] = a.Y + (int64_t)ids[b] * Dp;
        inv[j] = inv_norm(row_dot(yb[j], yb[j], Dp));
      } else {
        inv[j] = inv_norm(G[(size_t)b * P + b]);
      }
      smax = fmaxf(smax, base[j]);
      smin = fminf(smin, base[j]);
    }
  }
  int p = __popc(alive);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    smax = fmaxf(smax, __shfl_xor(smax, o, 64));
    smin = fminf(smin, __shfl_xor(smin, o, 64));
    p += __shfl_xor(p, o, 64);
  }
  const float lam = a.lam, oml = 1.0f - lam;
  const float range = smax - smin;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    float rel = base[j];
    if (!a.raw) rel = range > 0.0f ? (base[j] - smin) / range : 0.0f;
    base[j] = lam * rel;
  }

  const int steps = p < k ? p : k;
  for (int t = 0; t < steps; ++t) {
    u64 best = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if ((alive >> j) & 1u) {
        const float pen = oml * mm[j];
        const float v = t == 0 ? base[j] + 0.0f : (base[j] - pen) + 0.0f;
        const u64 w = ((u64)score_key(v) << 32) | (0xFFFFFFFFu - (uint32_t)(lane + 64 * j));
        best = w > best ? w : best;
      }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u64 x = __shfl_xor(best, o, 64);
      best = x > best ? x : best;
    }
    const int s = (int)(0xFFFFFFFFu - (uint32_t)best);  // < P: some slot is alive
    if (lane == 0) {
      items[t] = ids[s];
      scores[t] = sc[s];
      if (mmr) mmr[t] = score_unkey((uint32_t)(best >> 32));
    }
    if ((s & 63) == lane) alive &= ~(1u << (s >> 6));
    if (t + 1 == steps) break;
    if constexpr (LAZY) {
      const float* ys = a.Y + (int64_t)ids[s] * Dp;
      const float inv_s = inv_norm(row_dot(ys, ys, Dp));
      float g[NS];
#pragma unroll
      for (int j = 0; j < NS; ++j) g[j] = 0.0f;
#pragma unroll 1
      for (int c = 0; c < Dp; c += 4) {
        const float4 u = *reinterpret_cast<const float4*>(ys + c);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          const float4 v = *reinterpret_cast<const float4*>(yb[j] + c);
          g[j] = __builtin_fmaf(u.x, v.x, g[j]);
          g[j] = __builtin_fmaf(u.y, v.y, g[j]);
          g[j] = __builtin_fmaf(u.z, v.z, g[j]);
          g[j] = __builtin_fmaf(u.w, v.w, g[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const float cs = (g[j] * inv_s) * inv[j] + 0.0f;
        mm[j] = fmaxf(mm[j], cs);
      }
    } else {
      const float* gs = G + (size_t)s * P;
      const float inv_s = inv_norm(gs[s]);
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const int b = lane + 64 * j;
        if (b < P) {
          const float cs = (gs[b] * inv_s) * inv[j] + 0.0f;
          mm[j] = fmaxf(mm[j], cs);
        }
      }
    }
  }
  for (int t = steps + lane; t < k; t += 64) {
    items[t] = -1;
    scores[t] = -FLT_MAX;
    if (mmr) mmr[t] = -FLT_MAX;
  }
}

bool div_args_ok(const DiversifyArgs& a) {
  return a.pool >= 1 && a.pool <= kDiversifyMaxPool && a.k >= 1 && a.k <= a.pool && a.Dp >= 4 &&
         (a.Dp & 3) == 0 && a.Y && a.ids && a.pool_scores && (a.G || a.lazy) && a.out_items &&
         a.out_scores;
}

}  // namespace

hipError_t launch_diversify_gram(const DiversifyArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (!div_args_ok(a) || !a.G) return hipErrorInvalidValue;
  const int TB = (a.pool + 63) / 64, NB = TB * (TB + 1) / 2;
  const int groups = (NB + kGramWaves - 1) / kGramWaves;
  if (a.n > (int64_t)0x7fffffff / groups) return hipErrorInvalidValue;
  hipLaunchKernelGGL(div_gram_kernel, dim3((unsigned)(a.n * groups)), dim3(64 * kGramWaves), 0, s,
                     a, groups);
  return hipGetLastError();
}

hipError_t launch_diversify_select(const DiversifyArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (!div_args_ok(a) || (a.n + 3) / 4 > (int64_t)0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.n + 3) / 4)), block(256);
  const int ns = (a.pool + 63) / 64;
  if (a.lazy) {
    if (ns <= 1)
      hipLaunchKernelGGL((div_select_kernel<1, true>), grid, block, 0, s, a);
    else if (ns <= 2)
      hipLaunchKernelGGL((div_select_kernel<2, true>), grid, block, 0, s, a);
    else if (ns <= 4)
      hipLaunchKernelGGL((div_select_kernel<4, true>), grid, block, 0, s, a);
    else if (ns <= 8)
      hipLaunchKernelGGL((div_select_kernel<8, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((div_select_kernel<16, true>), grid, block, 0, s, a);
  } else {
    if (ns <= 1)
      hipLaunchKernelGGL((div_select_kernel<1, false>), grid, block, 0, s, a);
    else if (ns <= 2)
      hipLaunchKernelGGL((div_select_kernel<2, false>), grid, block, 0, s, a);
    else if (ns <= 4)
      hipLaunchKernelGGL((div_select_kernel<4, false>), grid, block, 0, s, a);
    else if (ns <= 8)
      hipLaunchKernelGGL((div_select_kernel<8, false>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((div_select_kernel<16, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace frecsys_hip
