// quality.hip -- list quality of ranked lists that are still in device memory
// (frecsys_rank_quality, frecsys_lists_quality): intra-list diversity (ILD),
// novelty and item exposure per cut-off.  A row has list_k slots of item ids, a
// negative id is an empty slot, a repeated id is a slot of its own; the
// definitions are include/frecsys_hip.h's, and frecsys_list_quality (serve.hip)
// is the same in scalar C++.
//
//   quality_kernel   one wave per row, four rows per workgroup.  The wave first
//                    closes the row's filled slots up into LDS (one ballot per
//                    64 positions; lane q < nk counts the filled slots below
//                    its own cut-off on the way), with each slot's weight
//                    beside its id.  Then one sweep in list order: lane l owns
//                    columns 4 l .. 4 l + 3 of every 256-column piece of the
//                    padded dim (one 16-byte load per piece; at Dp < 256 the
//                    upper lanes idle) and keeps its part of the running sum
//                    s = sum of the normalised rows so far in float64.  Per
//                    slot: the lane's parts of y.y and y.s, ONE joint xor
//                    butterfly for both, inv = 1 / sqrt(y.y), C += inv (y.s),
//                    s += inv y, W += weight.  The item rows of the next
//                    kAhead slots are in flight meanwhile: the ids are known up
//                    front, so the gathers never wait for the serial step (the
//                    pattern of cg_kernel's ids one chunk ahead).  Lane q keeps
//                    (C, W) as they stand after its cut-off's last filled slot.
//                    O(K d) per row for every cut-off at once; no K x K Gramian.
//   exposure_kernel  one thread per (row, position): a filled slot adds 1 to
//                    counts[q][id] for every cut-off above its position, with
//                    64-bit integer vector atomics -- exact, so the order of
//                    arrival does not matter.
//
// Fixed order: a lane adds its columns in ascending order, the butterfly pairs
// lanes at distances 32, 16, .. 1 (every lane ends with the same bits: the adds
// commute), the slots come in list order.  So a row's ILD and novelty bytes are
// a function of the padded dim, the item rows and the list alone -- not of the
// batch, the grid or the other rows.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;

constexpr int kRowsPerBlock = 4;
// Item rows in flight per wave ahead of the dependent step.  Four is the depth
// at which whole-row register gathers are known to reach the memory rate with
// 16 waves per CU; it was not swept here.  Registers allow 28 / 16 / 12 waves
// per CU for NV = 1 / 2 / 4, and the dynamic LDS (32 KiB per workgroup at
// K = 1024) caps a CU at 20 waves at the K limit.
constexpr int kAhead = 4;

template <int NV>
__global__ void __launch_bounds__(64 * kRowsPerBlock) quality_kernel(QualityArgs a) {
  extern __shared__ __align__(16) int32_t q_lds[];  // [rows per block][2][kpad]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  if (row >= a.n) return;  // the whole wave; no workgroup barrier below
  const int kpad = (a.k + 63) & ~63;
  int32_t* ids = q_lds + wave * 2 * kpad;
  float* wts = reinterpret_cast<float*>(ids + kpad);
  const int32_t* __restrict__ list = a.lists + row * a.list_k;
  const int kq = lane < a.nk ? a.k_list[lane] : 0;  // 1 .. a.k
  int nq = 0;  // filled slots below the lane's cut-off
  int n = 0;   // filled slots of the row
  for (int t = 0; t * 64 < a.k; ++t) {
    const int j = t * 64 + lane;
    const int32_t id = j < a.k ? list[j] : -1;
    const bool filled = id >= 0;
    const u64 mask = __ballot(filled);
    if (filled) {
      const int r = n + __popcll(mask & ((1ull << lane) - 1ull));  // < a.k <= kpad
      ids[r] = id;
      wts[r] = a.weight ? a.weight[id] : 0.0f;
    }
    const int left = kq - t * 64;
    if (left > 0) nq += __popcll(left >= 64 ? mask : (mask & ((1ull << left) - 1ull)));
    n += __popcll(mask);
  }
  n = __builtin_amdgcn_readfirstlane(n);
  wave_lds_sync();

  double C = 0.0, W = 0.0, Cq = 0.0, Wq = 0.0;
  if (a.ild) {
    const bool live = 4 * lane < a.Dp;  // every lane when Dp >= 256
    const float* __restrict__ ybase = a.Y + 4 * lane;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 y[kAhead][NV];
    double s[NV][4];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[v][e] = 0.0;
#pragma unroll
    for (int p = 0; p < kAhead; ++p)
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        y[p][v] = zero;
        if (p < n && live)
          y[p][v] = *reinterpret_cast<const float4*>(ybase + (int64_t)ids[p] * a.Dp + 256 * v);
      }
#pragma unroll 1
    for (int b0 = 0; b0 < n; b0 += kAhead) {
#pragma unroll
      for (int p = 0; p < kAhead; ++p) {
        const int b = b0 + p;
        if (b >= n) break;  // wave-uniform
        double yd[NV][4];
        double yy = 0.0, ys = 0.0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          yd[v][0] = (double)y[p][v].x;
          yd[v][1] = (double)y[p][v].y;
          yd[v][2] = (double)y[p][v].z;
          yd[v][3] = (double)y[p][v].w;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            yy = fma(yd[v][e], yd[v][e], yy);
            ys = fma(yd[v][e], s[v][e], ys);
          }
        }
        // the slot's registers are free: its successor kAhead slots on
        if (b + kAhead < n && live) {
          const float* src = ybase + (int64_t)ids[b + kAhead] * a.Dp;
#pragma unroll
          for (int v = 0; v < NV; ++v)
            y[p][v] = *reinterpret_cast<const float4*>(src + 256 * v);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          yy += __shfl_xor(yy, m, 64);
          ys += __shfl_xor(ys, m, 64);
        }
        const double inv = yy > 0.0 ? 1.0 / sqrt(yy) : 0.0;
        C += inv * ys;
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
          for (int e = 0; e < 4; ++e) s[v][e] = fma(inv, yd[v][e], s[v][e]);
        W += (double)wts[b];
        if (nq == b + 1) {
          Cq = C;
          Wq = W;
        }
      }
    }
  } else {
    for (int b = 0; b < n; ++b) {
      W += (double)wts[b];
      if (nq == b + 1) Wq = W;
    }
  }
  if (lane >= a.nk) return;
  const int64_t o = row * a.nk + lane;
  if (a.ild) {
    const double pairs = (double)((int64_t)nq * (nq - 1) / 2);
    a.ild[o] = nq >= 2 ? (float)(1.0 - Cq / pairs) : 0.0f;
  }
  if (a.novelty) a.novelty[o] = nq >= 1 ? (float)(Wq / (double)nq) : 0.0f;
}

__global__ void __launch_bounds__(256) exposure_kernel(ExposureArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n * a.k) return;
  const int64_t row = t / a.k;
  const int j = (int)(t - row * a.k);
  const int32_t id = a.lists[row * a.list_k + j];
  if (id < 0 || id >= a.m) return;  // an empty slot (an id beyond the table is the caller's fault)
  for (int q = 0; q < a.nk; ++q)
    if (j < a.k_list[q]) atomicAdd(a.counts + (int64_t)q * a.m + id, 1ull);
}

bool list_shape_ok(int64_t n, int list_k, int k, int nk, const void* lists, const void* k_list) {
  return n > 0 && k >= 1 && k <= kMetricMaxK && list_k >= k && nk >= 1 &&
         nk <= kMetricMaxCutoffs && lists && k_list;
}

}  // namespace

hipError_t launch_quality(const QualityArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (!list_shape_ok(a.n, a.list_k, a.k, a.nk, a.lists, a.k_list) || (!a.ild && !a.novelty) ||
      (a.novelty && !a.weight))
    return hipErrorInvalidValue;
  // the padded dims: a multiple of 4 up to 256 (one piece), 512, 1024
  if (a.ild && (!a.Y || a.Dp < 4 || (a.Dp & 3) || (a.Dp > 256 && a.Dp != 512 && a.Dp != 1024)))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.n + kRowsPerBlock - 1) / kRowsPerBlock)), block(64 * kRowsPerBlock);
  const size_t lds = (size_t)kRowsPerBlock * 2 * ((a.k + 63) & ~63) * sizeof(int32_t);
  if (a.Dp <= 256)
    hipLaunchKernelGGL(quality_kernel<1>, grid, block, lds, s, a);
  else if (a.Dp <= 512)
    hipLaunchKernelGGL(quality_kernel<2>, grid, block, lds, s, a);
  else
    hipLaunchKernelGGL(quality_kernel<4>, grid, block, lds, s, a);
  return hipGetLastError();
}

hipError_t launch_exposure(const ExposureArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (!list_shape_ok(a.n, a.list_k, a.k, a.nk, a.lists, a.k_list) || a.m < 1 || !a.counts)
    return hipErrorInvalidValue;
  const int64_t blocks = (a.n * a.k + 255) / 256;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(exposure_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace frecsys_hip
