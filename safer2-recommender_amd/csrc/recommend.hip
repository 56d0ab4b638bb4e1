// recommend.hip -- fused scoring + streaming top-K on gfx950: the serving
// path behind frecsys_recommend.  For a list of query rows x_r of a factor
// table and the item table V it returns, per row, the k best eligible items
// by (score descending, item id ascending) with their scores s = V x_r.  No
// rows x items score buffer exists: a workgroup keeps, per query row, only
// the candidates that can still be among the k best.
//
//   rec_history_kernel  bit j of bitmap[row] = 1 for every j of the row's CSR
//                       history (file order, repeats allowed): atomicOr;
//   rec_scan_kernel     grid (64-row blocks) x (item splits).  A workgroup
//                       sweeps the 128-item tiles of its split in ascending
//                       id: 64 x 128 scores per tile by v_mfma_f32_32x32x2_f32
//                       (score_kernel's tile, K in 32-wide slabs through LDS;
//                       the operands swapped, so that a lane holds scores of
//                       one query row and tests them against that row's
//                       threshold in registers),
//                       then appends the eligible (key, id) pairs that beat
//                       the row's threshold to the row's candidate buffer in
//                       HBM / L2, and compacts a buffer to its best k (one
//                       wave per row, bitonic sort in LDS) before a further
//                       tile could overflow it.
//                       Its SIM instantiation is the scan behind
//                       frecsys_similar (X = Y = one table): the scores are
//                       scaled by the two rows' inverse norms before they
//                       become keys (cosine), and a query row never appends
//                       its own id;
//   rec_merge_kernel    one workgroup per row: the best k of the splits'
//                       candidates, ids and scores out, -1 / -FLT_MAX in the
//                       slots beyond the eligible count.
//
// A candidate is one 64-bit word, key << 32 | ~id (key = score_key(score)):
// descending order of the words is score descending, then id ascending, and
// the words of one row are all different.  So every selection below is a
// selection of the largest words of a set, whatever order they were appended
// in, and the result does not depend on the split, the batch or the timing of
// the atomics.  Each score is the k-ascending fp32 FMA chain of the MFMA from
// +0 (cdna: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C))) over the padded dim (pad
// columns are zero: they add +0), the same in every tile, split and batch.
//
// Threshold invariant: a row's threshold is set only when its buffer is
// compacted at count >= k, between two tiles, to the key of the k-th best
// word of the tiles swept so far; a candidate of a later tile is appended
// only when key > threshold, strictly.  That is exact BECAUSE the sweep
// visits ids in ascending order: a later candidate with the SAME key has a
// larger id than each of the k kept ones, so its word is smaller than the
// k-th best and it could never be listed; with any other order of the ids a
// tie with the k-th key would have to be kept.  (Inside one tile the appends
// are unordered, but the threshold does not move there.  Stored as key + 1
// with the test key >= that, so that 0 means "no threshold yet".)  The SIM
// scan keeps the invariant: it sweeps ids ascending too, and its keys are
// those of the final, scaled score.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "common.h"
#include "kernels.h"
#include "scan_words.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;

constexpr int RT = 64;            // query rows per workgroup
constexpr int IT = 128;           // items per tile
constexpr int kMergeSlots = 8192;  // 64 KiB of candidates in the merge kernel's LDS
constexpr int kMaxSplits = 64;

__global__ void __launch_bounds__(64)
    rec_history_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                       const int64_t* __restrict__ qrows, int64_t r0, int64_t m, int64_t W,
                       uint32_t* __restrict__ bitmap) {
  const int64_t u = blockIdx.x;
  const int64_t e = qrows ? qrows[r0 + u] : r0 + u;
  const int64_t p0 = row_ptr[e], p1 = row_ptr[e + 1];
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 64) {
    const int64_t j = col[p];
    if (j >= 0 && j < m) atomicOr(&bitmap[u * W + (j >> 5)], 1u << (j & 31));
  }
}

// (compact_row, the cut of a candidate buffer to its best k: scan_words.h)

// The staging tiles and the four waves' sort slices share one LDS region: a
// wave sorts only between the barrier that ends a tile's appends (every MFMA
// read of xs / ys is done) and the barrier that opens the next tile's first
// k-slab (no wave stages before every wave has arrived there).
constexpr int kStageFloats = RT * 33 + 32 * (IT + 1);
// SIM = false is frecsys_recommend's scan.  SIM = true (frecsys_similar) reads
// a.inv / a.skip_self, which the other instantiation never touches: with
// a.inv the key is that of (dot * inv[query]) * inv[id] + 0.0f, two fp32
// multiplies in that order (the + 0.0f turns a -0.0 product into +0, which
// the dot chain never yields), and with a.skip_self the row's own id is
// cleared from the tile's eligibility word.
template <int CAP, bool SIM>
// 512 slots: registers for 4 waves per SIMD (4 workgroups of 27 KB per CU; the
// k-slab staging is latency-bound).  The larger sort slices allow 3 and 2.
__global__ void __launch_bounds__(256, CAP == 512 ? 4 : (CAP == 1024 ? 3 : 2))
    rec_scan_kernel(RecommendArgs a, int64_t W) {
  constexpr int kSortBytes = 4 * CAP * 8, kStageBytes = kStageFloats * 4;
  __shared__ __attribute__((aligned(16))) char
      lds[kSortBytes > kStageBytes ? kSortBytes : kStageBytes];
  float* xs = reinterpret_cast<float*>(lds);
  float* ys = xs + RT * 33;
  u64* sortbuf = reinterpret_cast<u64*>(lds);
  __shared__ uint32_t tkey[RT];  // a candidate passes with key >= tkey (0: no threshold yet)
  __shared__ int cnt[RT];
  __shared__ uint32_t elig[RT * 4];
  __shared__ int64_t xrow[RT];
  __shared__ u64* cbase[RT];  // the row's candidate buffer of this split
  __shared__ float yinv[SIM ? IT : 1];  // SIM: inverse norms of the tile's ids
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t base = (int64_t)blockIdx.x * RT;
  const int split = blockIdx.y, splits = a.splits;
  const int64_t ntiles = (a.m + IT - 1) / IT;
  const int64_t t0 = split * ntiles / splits, t1 = (split + 1) * ntiles / splits;
  const int Dp = a.Dp;
  const int R = wave & 1, Cs = (wave >> 1) * 2;
  if (tid < RT) {
    const int64_t row = base + tid;
    xrow[tid] = row < a.n ? (a.qrows ? a.qrows[a.r0 + row] : a.r0 + row) : -1;
    cnt[tid] = 0;
    cbase[tid] = a.cand + ((base + tid) * splits + split) * CAP;  // used for rows < n only
    tkey[tid] = row < a.n ? 0u : 0xffffffffu;
  }
  __syncthreads();
  const int NC = (Dp + 31) >> 5;
  const int rl = 32 * R + lo;  // the lane's query row in the block
  u64* const mycand = a.cand + ((base + rl) * splits + split) * CAP;
  float inv_q = 0.0f;  // SIM: the inverse norm of the lane's query row,
  int64_t self = -1;   // and the id it never lists
  if constexpr (SIM) {
    const int64_t xr = xrow[rl];
    if (a.inv && xr >= 0) inv_q = a.inv[xr];
    if (a.skip_self) self = xr;
  }
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t j0 = tile * IT;
    {  // eligibility words of the tile: 4 per row (the readers of the last
       // tile's words are past the barrier that ended its appends)
      const int rr = tid >> 2, w = tid & 3;
      uint32_t word = 0;
      if (xrow[rr] >= 0) {
        word = a.maskw[tile * 4 + w];
        if (a.bitmap) word &= ~a.bitmap[(base + rr) * W + tile * 4 + w];
      }
      elig[tid] = word;
      if constexpr (SIM) {
        if (a.inv && tid < IT) yinv[tid] = j0 + tid < a.m ? a.inv[j0 + tid] : 0.0f;
      }
    }
    f32x16 acc[2] = {f32x16{0.f}, f32x16{0.f}};
    for (int c = 0; c < NC; ++c) {
      __syncthreads();
      for (int s = tid; s < RT * 32; s += 256) {
        const int rr = s >> 5, kk = s & 31, col = 32 * c + kk;
        const int64_t xr = xrow[rr];
        xs[rr * 33 + kk] = (xr >= 0 && col < Dp) ? a.X[xr * Dp + col] : 0.0f;
      }
      for (int s = tid; s < 32 * IT; s += 256) {
        const int j = s >> 5, kk = s & 31, col = 32 * c + kk;
        const int64_t it = j0 + j;
        ys[kk * (IT + 1) + j] = (it < a.m && col < Dp) ? a.Y[it * Dp + col] : 0.0f;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int C = Cs + t;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
          const int kk = 2 * s2 + hi;
          // items as the MFMA's A rows, query rows as its B columns: the
          // accumulator holds S^T, a lane the scores of ONE query row
          acc[t] = mfma32(ys[kk * (IT + 1) + 32 * C + lo], xs[(32 * R + lo) * 33 + kk], acc[t]);
        }
      }
    }
    // append: lane (lo, hi) holds, for query row 32 R + lo, the 16 items
    // 32 C + acc_row(q, hi) of each of its two item blocks.  Threshold,
    // eligibility word and buffer are the lane's own row's: one LDS read
    // each per block, one atomic per lane and block that has a candidate.
    {
      const uint32_t tk = tkey[rl];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int C = Cs + t;
        uint32_t ew = elig[rl * 4 + C];
        if constexpr (SIM) {
          const int64_t so = self - (j0 + 32 * C);
          if (so >= 0 && so < 32) ew &= ~(1u << so);
          if (a.inv) {
#pragma unroll
            for (int q = 0; q < 16; ++q)
              acc[t][q] = __fadd_rn(
                  __fmul_rn(__fmul_rn(acc[t][q], inv_q), yinv[32 * C + acc_row(q, hi)]), 0.0f);
          }
        }
        uint32_t pm = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (score_key(acc[t][q]) >= tk && ((ew >> acc_row(q, hi)) & 1u)) pm |= 1u << q;
        if (pm) {
          int slot = atomicAdd(&cnt[rl], __popc(pm));
          const uint32_t id0 = (uint32_t)(j0 + 32 * C);
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            if ((pm >> q) & 1u) {
              // slot < CAP always: a row enters a tile with cnt <= CAP - IT
              if (slot < CAP)
                mycand[slot] = ((u64)score_key(acc[t][q]) << 32) | ~(id0 + acc_row(q, hi));
              ++slot;
            }
          }
        }
      }
    }
    __syncthreads();
    // a buffer that the next tile could overflow is cut to its best k
    for (int i = 0; i < RT / 4; ++i) {
      const int r = wave + 4 * i;
      const int nn = cnt[r];
      if (nn > CAP - IT) {  // wave-uniform
        u64 kth = 0ull;
        const int keep = compact_row<CAP>(cbase[r],
                                          sortbuf + wave * CAP, nn, a.k, lane, &kth);
        if (lane == 0) {
          cnt[r] = keep;
          if (nn >= a.k) tkey[r] = (uint32_t)(kth >> 32) + 1u;
        }
      }
    }
  }
  __syncthreads();
  for (int i = 0; i < RT / 4; ++i) {
    const int r = wave + 4 * i;
    if (base + r >= a.n) continue;
    u64 kth = 0ull;
    const int keep = compact_row<CAP>(cbase[r],
                                      sortbuf + wave * CAP, cnt[r], a.k, lane, &kth);
    if (lane == 0) a.counts[(base + r) * splits + split] = keep;
  }
}

__global__ void __launch_bounds__(256) rec_merge_kernel(RecommendArgs a, int64_t cap) {
  __shared__ u64 mb[kMergeSlots];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int splits = a.splits, k = a.k;
  int total = 0;
  for (int s = 0; s < splits; ++s) {
    int c = a.counts[row * splits + s];
    if (c > k) c = k;
    if (total + c > kMergeSlots) c = kMergeSlots - total;  // never: splits * k <= kMergeSlots
    const u64* g = a.cand + (row * splits + s) * cap;
    for (int i = tid; i < c; i += 256) mb[total + i] = g[i];
    total += c;
  }
  int P = 1;
  while (P < total) P <<= 1;
  for (int i = total + tid; i < P; i += 256) mb[i] = 0ull;
  __syncthreads();
  if (splits > 1) {  // one split: its list is already sorted
    for (int size = 2; size <= P; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int p = tid; p < (P >> 1); p += 256) {
          const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
          const int j = i | stride;
          const bool up = (i & size) == 0;
          const u64 x = mb[i], y = mb[j];
          if (up ? x < y : x > y) {
            mb[i] = y;
            mb[j] = x;
          }
        }
        __syncthreads();
      }
    }
  }
  for (int i = tid; i < k; i += 256) {
    const u64 v = i < total ? mb[i] : 0ull;
    a.out_items[row * k + i] = v ? (int32_t)~(uint32_t)v : -1;
    if (a.out_scores) a.out_scores[row * k + i] = v ? score_unkey((uint32_t)(v >> 32)) : -FLT_MAX;
  }
}

template <int CAP>
void launch_cap(const RecommendArgs& a, int64_t W, hipStream_t s) {
  const dim3 grid((unsigned)((a.n + RT - 1) / RT), (unsigned)a.splits);
  if (a.inv || a.skip_self)
    hipLaunchKernelGGL((rec_scan_kernel<CAP, true>), grid, dim3(256), 0, s, a, W);
  else
    hipLaunchKernelGGL((rec_scan_kernel<CAP, false>), grid, dim3(256), 0, s, a, W);
  hipLaunchKernelGGL(rec_merge_kernel, dim3((unsigned)a.n), dim3(256), 0, s, a, (int64_t)CAP);
}

}  // namespace

int recommend_cap(int k) {
  int cap = 512;
  while (cap < 4 * k && cap < 2048) cap <<= 1;
  return cap;
}

int64_t recommend_words(int64_t m) { return 4 * ((m + IT - 1) / IT); }

int recommend_max_splits(int k, int64_t m) {
  const int64_t ntiles = (m + IT - 1) / IT;
  int64_t s = kMergeSlots / (k < 1 ? 1 : k);
  if (s > kMaxSplits) s = kMaxSplits;
  if (s > ntiles) s = ntiles;
  return s < 1 ? 1 : (int)s;
}

hipError_t launch_history_bits(const int64_t* row_ptr, const int32_t* col, const int64_t* qrows,
                               int64_t r0, int64_t n, int64_t m, uint32_t* bitmap, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!row_ptr || !col || !bitmap || m < 1) return hipErrorInvalidValue;
  const int64_t W = recommend_words(m);
  hipError_t e = hipMemsetAsync(bitmap, 0, sizeof(uint32_t) * (size_t)n * (size_t)W, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rec_history_kernel, dim3((unsigned)n), dim3(64), 0, s, row_ptr, col, qrows, r0,
                     m, W, bitmap);
  return hipGetLastError();
}

hipError_t launch_recommend_merge(const RecommendArgs& a, int64_t cap, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.k < 1 || a.k > 1024 || a.splits < 1 || (int64_t)a.splits * a.k > kMergeSlots ||
      cap < a.k || !a.cand || !a.counts || !a.out_items)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(rec_merge_kernel, dim3((unsigned)a.n), dim3(256), 0, s, a, cap);
  return hipGetLastError();
}

hipError_t launch_recommend(const RecommendArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.k < 1 || a.k > 1024 || a.m < 1 || a.splits < 1 ||
      a.splits > recommend_max_splits(a.k, a.m) || !a.X || !a.Y || !a.maskw || !a.cand ||
      !a.counts || !a.out_items)
    return hipErrorInvalidValue;
  const int64_t W = recommend_words(a.m);
  if (a.bitmap) {
    if (!a.row_ptr || !a.col) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.bitmap, 0, sizeof(uint32_t) * (size_t)a.n * (size_t)W, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rec_history_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a.row_ptr, a.col,
                       a.qrows, a.r0, a.m, W, a.bitmap);
  }
  switch (recommend_cap(a.k)) {
    case 512: launch_cap<512>(a, W, s); break;
    case 1024: launch_cap<1024>(a, W, s); break;
    default: launch_cap<2048>(a, W, s); break;
  }
  return hipGetLastError();
}

}  // namespace frecsys_hip
