// similar.hip -- the norm pass behind frecsys_similar (nearest neighbours of
// rows of one factor table T among the rows of T, by dot product or cosine).
// The scan is recommend.hip's: rec_scan_kernel<CAP, true> with X = Y = T, the
// scores scaled by the inverse norms computed here, the query's own id cleared
// from its eligibility bits.
//
//   row_inv_norm_kernel  one lane per row: n2 = the fp32 chain acc =
//                        fmaf(T[r][c], T[r][c], acc) over the padded dim in
//                        ascending c from +0, then inv = n2 > 0 ?
//                        1 / sqrt(n2) : 0 (sqrt and division correctly
//                        rounded).
//
// The chain is the scan's own score of row r with itself, bit for bit (the
// MFMA's k-ascending FMA chain; rerank.hip relies on the same identity), not a
// tree: so the cosine of a row with itself, or with a row equal in value, is
// (n2 * inv) * inv of one and the same n2 and inv, and inv depends on row r
// and Dp alone -- not on the batch, the split or the grid.  A lane walks its
// row in float4s (Dp is a multiple of 8); a wave's 64 rows are 64 streams of
// whole cache lines.  The pass reads the table once, m Dp 4 bytes, against the
// scan's n m Dp 2 flops.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

__global__ void __launch_bounds__(256)
    row_inv_norm_kernel(const float* __restrict__ T, int64_t m, int Dp, float* __restrict__ inv) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const float4* __restrict__ row = reinterpret_cast<const float4*>(T + r * Dp);
  float acc = 0.0f;
  for (int c = 0; c < (Dp >> 2); ++c) {
    const float4 v = row[c];
    acc = __fmaf_rn(v.x, v.x, acc);
    acc = __fmaf_rn(v.y, v.y, acc);
    acc = __fmaf_rn(v.z, v.z, acc);
    acc = __fmaf_rn(v.w, v.w, acc);
  }
  inv[r] = acc > 0.0f ? __fdiv_rn(1.0f, __fsqrt_rn(acc)) : 0.0f;
}

}  // namespace

hipError_t launch_row_inv_norm(const float* T, int64_t m, int Dp, float* inv, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  if (!T || !inv || Dp < 4 || (Dp & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(row_inv_norm_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, T, m,
                     Dp, inv);
  return hipGetLastError();
}

}  // namespace frecsys_hip
