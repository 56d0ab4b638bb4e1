// explain.hip -- a score split exactly over the history entries (frecsys_explain).
//
// Every user projection of frecsys_solve_side (kinds IALS and WEIGHTED_U)
// solves A x = b with
//   A = s_G G + sum_j c_j y_j y_j^T + lambda I,   b = sum_j c_j y_j
// over the history rows y_j (the table of cg.hip's header: iALS s_G = w,
// c_j = 1; WEIGHTED_U s_G = omega w, c_j = omega / h).  The score of a target
// item t is then v_t . x = sum_j contrib_j(t), contrib_j(t) = c_j y_j . w_t
// with w_t = A^-1 v_t.
//
// explain_kernel: one workgroup of 8 waves per query row at a time (the rows
// of the batch strided over the grid in the host's order, most work first).
//   1. Assemble.  S = sum_j y_j y_j^T on v_mfma_f32_32x32x2_f32 (exact fp32
//      products), the operands straight from the table: lane (lo, hi) of a
//      wave supplies element 32 I + lo of history row 2 s + hi, so a tile's
//      element is one accumulator chain over j ascending (rows past the
//      history add +0).  The T (T + 1) / 2 lower tiles are dealt round-robin
//      to the waves, one accumulator at a time, and A = assemble(kind, S, G,
//      ...) (common.h, the solve kernels' own expression) goes to the
//      swizzled LDS tiles.  Dp = 8 / 16 run as one tile with a unit diagonal
//      behind the Dp-th row.
//   2. Factor.  chol_factor_tiles (chol.h): A = L L^T, diagonal tiles
//      inverted.  A failed pivot reports the entity and ends the row.
//   3. Substitute, per group of <= 32 targets: Z = V_g L^-T and W = Z L^-1
//      with the right-hand sides as target-major tiles (element (t, k) =
//      component k of target t).  Wave p keeps tile p in its accumulator
//      registers -- at T = 8 the 36 tiles of L take 144 KB of the 160 KB of
//      LDS and the 32 KB of right-hand sides do not fit beside them -- and
//      only the tile that has just become final goes through a 4 KB LDS
//      scratch tile, from which the other waves fold it into theirs
//      (right-looking; one barrier per block column; exact fp32 products,
//      tile_pqT / tile_pq).  The factor stays in LDS for the row's next group.
//   4. Second pass.  W goes to the workgroup's slot in global memory (32 KB
//      at most, read back through L2 by the same workgroup after a barrier);
//      the history is streamed again in chunks of kExplainChunk rows, 32 per
//      wave: contrib[t][j] = c_j sum_k w_t[k] y_j[k] as one 32 x 32 MFMA
//      accumulator per wave and chunk, both operands straight from global
//      memory, k ascending.
// explain_select_kernel: one wave per (row, target) pair.  score = the sum of
// the pair's contributions: lane l adds the entries j = l, l + 64, ... in
// ascending order from +0, then the 64 partial sums are folded by the
// butterfly over lane distances 1, 2, 4, .. 32.  The `top` largest by
// (contribution descending, CSR position ascending) by repeated maximum
// search over the 64-bit word (score_key(value) << 32 | ~position), -0
// ordered as +0.
//
// Every chain above is a function of the row's history, the parameters and
// the tables alone: a pair's bits do not depend on the batch, the grid, the
// other rows or targets, the grouping of the targets, `top` or the side.
#include <hip/hip_runtime.h>

#include "chol.h"
#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

constexpr int kExWaves = 8;
constexpr int kExThreads = 64 * kExWaves;
constexpr int kExU = 8;  // history row pairs in flight per wave in the assembly
static_assert(kExplainChunk == 32 * kExWaves, "one 32-row MFMA tile per wave and sweep");

__device__ __forceinline__ int ex_tiles(int Dp) { return Dp < 32 ? 1 : Dp / 32; }

__global__ void __launch_bounds__(kExThreads) explain_kernel(ExplainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Dp = a.Dp;
  const int T = ex_tiles(Dp), NT = T * (T + 1) / 2, LD = 32 * T;
  float* tiles = smem;
  float* S0 = tiles + NT * 1024;  // the owner's operand tile
  float* S1 = S0 + 1024;          // [2] the block just made final, double-buffered
  int* flag = reinterpret_cast<int*>(S1 + 2048);
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* wslot = a.wws + (size_t)blockIdx.x * kExplainGroup * LD;

  for (int64_t ii = blockIdx.x; ii < a.n; ii += gridDim.x) {
    const int64_t i = a.order[ii];  // longest first: the batch ends with short rows
    const int64_t e = a.qrows ? a.qrows[a.r0 + i] : a.r0 + i;
    const int64_t p0 = a.row_ptr[e], h = a.row_ptr[e + 1] - p0;
    const int64_t tp0 = a.tgt_ptr[a.r0 + i] - a.tgt_base;
    const int64_t m = a.tgt_ptr[a.r0 + i + 1] - a.tgt_ptr[a.r0 + i];
    if (h == 0 || m == 0) continue;  // workgroup-uniform
    const bool ukind = a.kind == KIND_WEIGHTED_U;
    const float omega = (ukind && a.entity_weight) ? a.entity_weight[e] : 1.0f;
    const float lam = entity_lambda(a.kind, a.reg, a.reg_exp, a.w, 0.0f, h, a.n_other, nullptr, e,
                                    a.lambda_is_reg);
    const float cu = ukind ? omega / (float)h : 1.0f;

    // ---- 1. assemble: this wave's lower tiles t = wave, wave + 8, ... ----
    if (tid == 0) flag[0] = 0;
#pragma unroll 1
    for (int t = wave; t < NT; t += kExWaves) {
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= t) ++I;
      const int J = t - I * (I + 1) / 2;
      const int ca = 32 * I + lo, cb = 32 * J + lo;
      const bool la = ca < Dp, lb = cb < Dp;
      f32x16 acc = f32x16{0.f};
      // kExU row pairs per step, their ids one step ahead of the rows
      int id[kExU], idn[kExU];
#pragma unroll
      for (int u = 0; u < kExU; ++u) id[u] = 2 * u + hi < h ? a.col[p0 + 2 * u + hi] : -1;
#pragma unroll 1
      for (int64_t k0 = 0; k0 < h; k0 += 2 * kExU) {
        float av[kExU], bv[kExU];
#pragma unroll
        for (int u = 0; u < kExU; ++u) {
          const float* yr = a.X + (int64_t)(id[u] < 0 ? 0 : id[u]) * Dp;
          av[u] = (id[u] >= 0 && la) ? yr[ca] : 0.0f;
          bv[u] = (id[u] >= 0 && lb) ? yr[cb] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kExU; ++u) {
          const int64_t kn = k0 + 2 * kExU + 2 * u + hi;
          idn[u] = kn < h ? a.col[p0 + kn] : -1;
        }
#pragma unroll
        for (int u = 0; u < kExU; ++u) {
          acc = mfma32(av[u], bv[u], acc);
          id[u] = idn[u];
        }
      }
      float* At = tiles + t * 1024;  // t = tidx(I, J)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = acc_row(q, hi);
        const int gi = 32 * I + r, gj = cb;
        float v;
        if (gi < Dp && gj < Dp)
          v = assemble(a.kind, acc[q], a.G[gi * Dp + gj], gi == gj, a.w, lam, (float)h, omega);
        else
          v = gi == gj ? 1.0f : 0.0f;  // Dp = 8 / 16: the unit diagonal of the padding
        At[sw(r, lo)] = v;
      }
    }
    __syncthreads();

    // ---- 2. factor ----
    chol_factor_tiles<kExWaves>(tiles, T, flag, tid);
    if (flag[0]) {  // workgroup-uniform (read behind the factor's last barrier)
      if (tid == 0) atomicMin(a.fail, (unsigned long long)(e + 1));
      __syncthreads();
      continue;
    }

    for (int64_t g0 = 0; g0 < m; g0 += kExplainGroup) {
      const int mg = (int)(m - g0 < kExplainGroup ? m - g0 : kExplainGroup);
      // ---- 3. substitute: wave p holds block p of the group's right-hand sides ----
      f32x16 c = f32x16{0.f};
      if (wave < T) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int t = acc_row(q, hi), k = 32 * wave + lo;
          if (t < mg && k < Dp) c[q] = a.X[(int64_t)a.tgt[tp0 + g0 + t] * Dp + k];
        }
      }
      // forward: Z_p = R_p L_pp^-T, then R_q -= Z_p L_qp^T for q > p
#pragma unroll 1
      for (int p = 0; p < T; ++p) {
        float* Z = S1 + (p & 1) * 1024;
        if (wave == p) {
#pragma unroll
          for (int q = 0; q < 16; ++q) S0[sw(acc_row(q, hi), lo)] = c[q];
          wave_lds_sync();
          c = tile_pqT(S0, tiles + tidx(p, p) * 1024, lo, hi);
#pragma unroll
          for (int q = 0; q < 16; ++q) Z[sw(acc_row(q, hi), lo)] = c[q];
        }
        lds_barrier();
        if (wave > p && wave < T) {
          const f32x16 u = tile_pqT(Z, tiles + tidx(wave, p) * 1024, lo, hi);
#pragma unroll
          for (int q = 0; q < 16; ++q) c[q] -= u[q];
        }
      }
      lds_barrier();
      // backward: W_p = R_p L_pp^-1, then R_q -= W_p L_pq for q < p
#pragma unroll 1
      for (int p = T - 1; p >= 0; --p) {
        float* Z = S1 + (p & 1) * 1024;
        if (wave == p) {
#pragma unroll
          for (int q = 0; q < 16; ++q) S0[sw(acc_row(q, hi), lo)] = c[q];
          wave_lds_sync();
          c = tile_pq(S0, tiles + tidx(p, p) * 1024, lo, hi);
#pragma unroll
          for (int q = 0; q < 16; ++q) Z[sw(acc_row(q, hi), lo)] = c[q];
        }
        lds_barrier();
        if (wave < p) {
          const f32x16 u = tile_pq(Z, tiles + tidx(p, wave) * 1024, lo, hi);
#pragma unroll
          for (int q = 0; q < 16; ++q) c[q] -= u[q];
        }
      }
      if (wave < T) {
#pragma unroll
        for (int q = 0; q < 16; ++q) wslot[acc_row(q, hi) * LD + 32 * wave + lo] = c[q];
      }
      __syncthreads();  // the slot's rows are visible to the workgroup

      // ---- 4. second pass: contrib[t][j] = c_j (w_t . y_j) ----
      float* cb = a.contrib + a.coff[i] + g0 * h;
      const int64_t nch = (h + 31) / 32;
      for (int64_t ch = wave; ch < nch; ch += kExWaves) {
        const int64_t j = 32 * ch + lo;
        const bool live = j < h;
        const int id = live ? a.col[p0 + j] : 0;
        const float* yr = a.X + (int64_t)id * Dp + 4 * hi;
        const float* wr = wslot + lo * LD + 4 * hi;
        f32x16 u = f32x16{0.f};
        for (int k0 = 0; k0 < Dp; k0 += 8) {
          const float4 wv = *reinterpret_cast<const float4*>(wr + k0);
          float4 yv = make_float4(0.f, 0.f, 0.f, 0.f);
          if (live) yv = *reinterpret_cast<const float4*>(yr + k0);
          u = mfma32(wv.x, yv.x, u);
          u = mfma32(wv.y, yv.y, u);
          u = mfma32(wv.z, yv.z, u);
          u = mfma32(wv.w, yv.w, u);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int t = acc_row(q, hi);
          if (t < mg && live) cb[(int64_t)t * h + j] = cu * u[q];
        }
      }
      __syncthreads();  // the slot is rewritten by the next group / row
    }
  }
}

// (value descending, position ascending) as one unsigned order; -0 as +0
__device__ __forceinline__ unsigned long long ex_word(float v, int64_t j) {
  v += 0.0f;  // -0 + +0 = +0
  return ((unsigned long long)score_key(v) << 32) | (0xFFFFFFFFu - (uint32_t)j);
}

__global__ void __launch_bounds__(256) explain_select_kernel(ExplainArgs a, int64_t n_pairs) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= n_pairs) return;  // wave-uniform
  const int64_t i = a.prow[pair];
  const int64_t e = a.qrows ? a.qrows[a.r0 + i] : a.r0 + i;
  const int64_t p0 = a.row_ptr[e], h = a.row_ptr[e + 1] - p0;
  const int64_t t = pair - (a.tgt_ptr[a.r0 + i] - a.tgt_base);
  const int top = a.top;
  int32_t* items = a.top_items + pair * top;
  float* vals = a.top_contrib + pair * top;
  const float* cb = a.contrib + a.coff[i] + t * h;
  float s = 0.0f;
  for (int64_t j = lane; j < h; j += 64) s += cb[j];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) a.score[pair] = s;
  unsigned long long prev = ~0ull;
  int r = 0;
  for (; r < top; ++r) {
    unsigned long long best = 0;
    for (int64_t j = lane; j < h; j += 64) {
      const unsigned long long w = ex_word(cb[j], j);
      if (w < prev && w > best) best = w;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long x = __shfl_xor(best, o, 64);
      best = x > best ? x : best;
    }
    if (best == 0) break;  // fewer than `top` entries
    const int64_t pos = (int64_t)(0xFFFFFFFFu - (uint32_t)best);
    if (lane == 0) {
      items[r] = a.col[p0 + pos];
      vals[r] = cb[pos];
    }
    prev = best;
  }
  for (int q = r + lane; q < top; q += 64) {
    items[q] = -1;
    vals[q] = 0.0f;
  }
}

}  // namespace

int explain_ld(int Dp) { return Dp < 32 ? 32 : Dp; }

size_t explain_lds_bytes(int Dp) {
  const int T = Dp < 32 ? 1 : Dp / 32;
  return sizeof(float) * (size_t)(T * (T + 1) / 2 + 3) * 1024 + 16;
}

hipError_t launch_explain(const ExplainArgs& a, int grid, hipStream_t s) {
  if (a.n <= 0 || grid <= 0) return hipSuccess;
  static bool attr = false;
  if (!attr) {
    hipError_t err = hipFuncSetAttribute((const void*)explain_kernel,
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)explain_lds_bytes(256));
    if (err != hipSuccess) return err;
    attr = true;
  }
  hipLaunchKernelGGL(explain_kernel, dim3((unsigned)grid), dim3(kExThreads),
                     explain_lds_bytes(a.Dp), s, a);
  return hipGetLastError();
}

hipError_t launch_explain_select(const ExplainArgs& a, int64_t n_pairs, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(explain_select_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0, s, a,
                     n_pairs);
  return hipGetLastError();
}

}  // namespace frecsys_hip
