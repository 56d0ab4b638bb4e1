// positions.hip -- exact full-catalogue positions of ground-truth items on
// gfx950: the kernels behind frecsys_rank_positions.  For query row i and a
// ground-truth item j the answer is the number of eligible items whose
// candidate word (score_key(score) << 32 | ~id, recommend.hip) is larger than
// j's: the 0-based slot frecsys_recommend would list j in if its k were large
// enough.  No rows x items score matrix, no candidate buffers, no top-K: the
// scan only counts.
//
//   pos_prepare_kernel  one workgroup per query row.  Thread t scores ground-
//                       truth entry t, t + 256, ... by frecsys_score_pairs'
//                       chain (acc = fmaf(v[c], x[c], acc), c ascending from
//                       +0 over the padded dim: the scan's score bit for bit),
//                       forms the word -- 0 when the item is masked out or in
//                       the row's history -- and keeps it per entry.  The
//                       words are then sorted descending (bitonic network, all
//                       comparators in one direction so that any length works
//                       without padding; in LDS up to kSortLds words, else in
//                       place in global memory), repeats are zeroed and the
//                       sort is run again: the row's g distinct eligible words
//                       lie first, as thresholds T[0 .. g).  The row's
//                       counters are zeroed;
//   pos_scan_kernel     grid (64-row blocks) x (item splits): rec_scan_kernel's
//                       tile -- 64 rows x 128 items, K in 32-wide slabs through
//                       LDS, v_mfma_f32_32x32x2_f32 with the items on the A
//                       side, so that a lane holds the scores of one query row
//                       -- with the same staging and the same k-ascending
//                       chain, which is what makes a scanned score equal a
//                       prepared one.  After a tile a lane tests each eligible
//                       score's word w against its row's smallest threshold;
//                       most end there.  A larger w finds b = |{q : T[q] >= w}|
//                       by binary search and increments counter b of the row:
//                       an integer atomicAdd, so neither order, split, batch
//                       nor timing can change a result.  Rows with g <=
//                       kPosLds keep thresholds and counters in LDS and flush
//                       the counters to global memory at the end of the split;
//                       a row with more searches its thresholds and counts in
//                       global memory / L2, as exactly;
//   pos_finish_kernel   one wave per row: inclusive prefix sum of the counters
//                       (rank of threshold q = counter[0] + ... + counter[q]:
//                       an item that is itself ground truth has q + 1
//                       thresholds >= its word, so it never counts against
//                       itself), rank[t] by binary search of entry t's word
//                       among the thresholds (-1 for a zero word), M = the
//                       popcount of the row's eligibility words, and mrr / auc
//                       by frecsys_position_metrics' own operations: int64
//                       sums, IEEE double divide and subtract, one conversion
//                       to float (the build has no fast-math flag).
//
// Limits.  kPosLds = 32 thresholds per row are LDS-resident in the scan (16.5
// KB of words and 8.25 KB of counters beside the 24.4 KB of staging: three
// workgroups per CU); kSortLds = 2048 words are sorted in LDS by the prepare
// kernel.  Neither bounds what is exact -- only where the data lives.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;

constexpr int RT = 64;          // query rows per workgroup
constexpr int IT = 128;         // items per tile
constexpr int kPosLds = 32;     // thresholds per row kept in the scan's LDS
constexpr int kCntLd = kPosLds + 1;
// row stride of the LDS thresholds, in words: odd, so that the lanes of a
// half-wave (32 rows) searching at the same depth read 32 different bank pairs
constexpr int kThrLd = kPosLds + 1;
constexpr int kSortLds = 2048;  // words the prepare kernel sorts in LDS
constexpr int kMaxSplits = 64;

// a[0 .. n) sorted descending by the 256 threads of a workgroup; a in LDS or
// global memory.  The bitonic network in its one-direction form: the first
// step of every merge pairs i with its mirror image in the block, the rest are
// half-cleaners, and every comparator leaves the larger word at the lower
// index.  A pad beyond n would be the smallest word at the higher index of
// each of its comparators and never move, so those comparators are skipped.
__device__ __forceinline__ void sort_desc(u64* a, int64_t n, int tid) {
  int64_t P = 1;
  while (P < n) P <<= 1;
  for (int64_t size = 2; size <= P; size <<= 1) {
    for (int64_t stride = size >> 1; stride > 0; stride >>= 1) {
      const bool mirror = stride == (size >> 1);
      for (int64_t p = tid; p < (P >> 1); p += 256) {
        const int64_t i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        const int64_t j = mirror ? (i ^ (size - 1)) : (i | stride);
        if (j < n) {
          const u64 x = a[i], y = a[j];
          if (x < y) {
            a[i] = y;
            a[j] = x;
          }
        }
      }
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(256) pos_prepare_kernel(PositionsArgs a, int64_t W) {
  __shared__ u64 sb[kSortLds];
  __shared__ __attribute__((aligned(16))) float xs[1024];
  __shared__ int gcount;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t xr = a.qrows ? a.qrows[a.r0 + row] : a.r0 + row;
  const int Dp = a.Dp;
  const int64_t p0 = a.gt_ptr[a.r0 + row] - a.gt_base;
  const int64_t len = a.gt_ptr[a.r0 + row + 1] - a.gt_base - p0;
  for (int c = tid; c < Dp; c += 256) xs[c] = a.X[xr * Dp + c];
  if (tid == 0) gcount = 0;
  uint32_t* const cnt = a.counters + p0 + row;  // len + 1 counters
  for (int64_t t = tid; t <= len; t += 256) cnt[t] = 0u;
  __syncthreads();
  u64* const s = len <= kSortLds ? sb : a.thr + p0;
  for (int64_t t = tid; t < len; t += 256) {
    const uint32_t id = (uint32_t)a.gt[p0 + t];
    const float* __restrict__ y = a.Y + (int64_t)id * Dp;
    float acc = 0.0f;
    for (int c = 0; c < Dp; c += 4) {
      const f32x4v v = *reinterpret_cast<const f32x4v*>(y + c);
      acc = fmaf(v[0], xs[c], acc);
      acc = fmaf(v[1], xs[c + 1], acc);
      acc = fmaf(v[2], xs[c + 2], acc);
      acc = fmaf(v[3], xs[c + 3], acc);
    }
    bool el = (a.maskw[id >> 5] >> (id & 31)) & 1u;
    if (el && a.bitmap) el = !((a.bitmap[row * W + (id >> 5)] >> (id & 31)) & 1u);
    const u64 word = el ? (((u64)score_key(acc) << 32) | (uint32_t)~id) : 0ull;
    a.words[p0 + t] = word;
    s[t] = word;
  }
  __syncthreads();
  sort_desc(s, len, tid);
  // a run of equal words keeps its last: the reads look ahead, where no word
  // has been zeroed yet
  for (int64_t b0 = 0; b0 < len; b0 += 256) {
    const int64_t i = b0 + tid;
    const bool dup = i + 1 < len && s[i] == s[i + 1];
    __syncthreads();
    if (dup) s[i] = 0ull;
  }
  __syncthreads();
  sort_desc(s, len, tid);
  int mine = 0;
  for (int64_t t = tid; t < len; t += 256) mine += s[t] != 0ull;
  if (mine) atomicAdd(&gcount, mine);
  __syncthreads();
  const int g = gcount;
  if (s == sb)
    for (int t = tid; t < g; t += 256) a.thr[p0 + t] = sb[t];
  if (tid == 0) a.g[row] = g;
}

// |{q < g : T[q] >= w}| for T descending.
__device__ __forceinline__ int count_ge(const u64* T, int g, u64 w) {
  int lo = 0, hi = g;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T[mid] >= w) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

constexpr int kStageFloats = RT * 33 + 32 * (IT + 1);

// 51.4 KB of LDS: three workgroups per CU, 3 waves per SIMD.
__global__ void __launch_bounds__(256, 3) pos_scan_kernel(PositionsArgs a, int64_t W) {
  __shared__ __attribute__((aligned(16))) float stage[kStageFloats];
  __shared__ u64 lthr[RT * kThrLd];
  __shared__ uint32_t lcnt[RT * kCntLd];
  __shared__ uint32_t elig[RT * 4];
  __shared__ int64_t xrow[RT];
  __shared__ int64_t loff[RT];  // the row's first threshold in a.thr
  __shared__ int lg[RT];        // thresholds of the row (0: none, or no row)
  float* xs = stage;
  float* ys = xs + RT * 33;
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
    const bool valid = row < a.n;
    xrow[tid] = valid ? (a.qrows ? a.qrows[a.r0 + row] : a.r0 + row) : -1;
    loff[tid] = valid ? a.gt_ptr[a.r0 + row] - a.gt_base : 0;
    lg[tid] = valid ? a.g[row] : 0;
  }
  for (int s = tid; s < RT * kCntLd; s += 256) lcnt[s] = 0u;
  __syncthreads();
  for (int s = tid; s < RT * kPosLds; s += 256) {
    const int rr = s / kPosLds, q = s % kPosLds, g = lg[rr];
    if (g <= kPosLds && q < g) lthr[rr * kThrLd + q] = a.thr[loff[rr] + q];
  }
  __syncthreads();
  const int NC = (Dp + 31) >> 5;
  const int rl = 32 * R + lo;  // the lane's query row in the block
  const int g = lg[rl];
  const bool in_lds = g <= kPosLds;
  const u64* const gthr = a.thr + loff[rl];
  uint32_t* const gcnt = a.counters + loff[rl] + (base + rl);
  // the smallest threshold: a word at or below it changes no rank
  const u64 tmin = g > 0 ? (in_lds ? lthr[rl * kThrLd + g - 1] : gthr[g - 1]) : ~0ull;
  const uint32_t kmin = (uint32_t)(tmin >> 32);
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t j0 = tile * IT;
    f32x16 acc[2] = {f32x16{0.f}, f32x16{0.f}};
    for (int c = 0; c < NC; ++c) {
      __syncthreads();
      if (c == 0) {
        // eligibility words of the tile: 4 per row.  Written here, between the
        // two barriers of the first slab: the barrier above is the first one
        // after the last tile's counting (which has none of its own), so every
        // reader of the last tile's words has passed it, and the barrier below
        // comes before this tile's counting reads them.
        const int rr = tid >> 2, w = tid & 3;
        uint32_t word = 0;
        if (xrow[rr] >= 0) {
          word = a.maskw[tile * 4 + w];
          if (a.bitmap) word &= ~a.bitmap[(base + rr) * W + tile * 4 + w];
        }
        elig[tid] = word;
      }
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
    // count: lane (lo, hi) holds, for query row 32 R + lo, the 16 items
    // 32 C + acc_row(q, hi) of each of its two item blocks
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int C = Cs + t;
      const uint32_t ew = elig[rl * 4 + C];
      const uint32_t id0 = (uint32_t)(j0 + 32 * C);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const uint32_t key = score_key(acc[t][q]);
        if (key >= kmin && ((ew >> acc_row(q, hi)) & 1u)) {
          const u64 w = ((u64)key << 32) | ~(id0 + acc_row(q, hi));
          if (w > tmin) {  // so b < g
            if (in_lds)
              atomicAdd(&lcnt[rl * kCntLd + count_ge(lthr + rl * kThrLd, g, w)], 1u);
            else
              atomicAdd(&gcnt[count_ge(gthr, g, w)], 1u);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < RT * kCntLd; s += 256) {
    const int rr = s / kCntLd, b = s % kCntLd, gr = lg[rr];
    if (gr <= kPosLds && b < gr) {
      const uint32_t v = lcnt[s];
      if (v) atomicAdd(&a.counters[loff[rr] + (base + rr) + b], v);
    }
  }
}

constexpr int kRowsPerBlock = 4;

__global__ void __launch_bounds__(64 * kRowsPerBlock)
    pos_finish_kernel(PositionsArgs a, int64_t W) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= a.n) return;  // the whole wave
  const int64_t p0 = a.gt_ptr[a.r0 + row] - a.gt_base;
  const int64_t len = a.gt_ptr[a.r0 + row + 1] - a.gt_base - p0;
  const int g = a.g[row];
  uint32_t* const cnt = a.counters + p0 + row;
  const u64* __restrict__ thr = a.thr + p0;
  // counter q becomes the rank of threshold q; inv = sum_q (rank_q - q)
  uint32_t carry = 0, first = 0;  // first: the best rank of the row
  long long inv = 0;
  for (int b0 = 0; b0 < g; b0 += 64) {
    const int i = b0 + lane;
    uint32_t incl = i < g ? cnt[i] : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    incl += carry;
    if (i < g) {
      cnt[i] = incl;
      inv += (long long)incl - (long long)i;
    }
    if (b0 == 0) first = __shfl(incl, 0);
    carry = __shfl(incl, 63);
  }
  __threadfence();  // the ranks are read below by other lanes of the wave
  for (int64_t t = lane; t < len; t += 64) {
    const u64 w = a.words[p0 + t];
    int32_t r = -1;
    if (w) {
      int lo = 0, hi = g;  // the q with thr[q] == w
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] > w) lo = mid + 1;
        else hi = mid;
      }
      r = (int32_t)cnt[lo];
    }
    a.rank[p0 + t] = r;
  }
  int M = 0;
  for (int64_t w = lane; w < W; w += 64) {
    uint32_t word = a.maskw[w];
    if (a.bitmap) word &= ~a.bitmap[row * W + w];
    M += __popc(word);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    M += __shfl_xor(M, o);
    const int ilo = __shfl_xor((int)(uint32_t)inv, o), ihi = __shfl_xor((int)(inv >> 32), o);
    inv += (long long)(((u64)(uint32_t)ihi << 32) | (uint32_t)ilo);
  }
  if (lane == 0) {
    a.eligible[row] = M;
    float mrr = 0.0f, auc = 0.0f;
    if (g > 0) {
      mrr = (float)(1.0 / (double)((long long)first + 1));
      auc = M == g ? 1.0f
                   : (float)(1.0 - (double)inv / ((double)g * (double)((long long)M - g)));
    }
    a.mrr[row] = mrr;
    a.auc[row] = auc;
  }
}

}  // namespace

int positions_lds_thresholds() { return kPosLds; }

int positions_max_splits(int64_t m) {
  const int64_t ntiles = (m + IT - 1) / IT;
  return (int)(ntiles < kMaxSplits ? (ntiles < 1 ? 1 : ntiles) : kMaxSplits);
}

hipError_t launch_positions(const PositionsArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.m < 1 || a.splits < 1 || a.splits > positions_max_splits(a.m) || !a.X || !a.Y ||
      !a.maskw || !a.gt_ptr || !a.gt || !a.words || !a.thr || !a.g || !a.counters || !a.rank ||
      !a.eligible || !a.mrr || !a.auc || a.Dp < 1 || a.Dp > 1024 || (a.Dp & 7))
    return hipErrorInvalidValue;
  const int64_t W = recommend_words(a.m);
  if (a.bitmap) {
    if (!a.row_ptr || !a.col) return hipErrorInvalidValue;
    const hipError_t e =
        launch_history_bits(a.row_ptr, a.col, a.qrows, a.r0, a.n, a.m, a.bitmap, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pos_prepare_kernel, dim3((unsigned)a.n), dim3(256), 0, s, a, W);
  hipLaunchKernelGGL(pos_scan_kernel, dim3((unsigned)((a.n + RT - 1) / RT), (unsigned)a.splits),
                     dim3(256), 0, s, a, W);
  hipLaunchKernelGGL(pos_finish_kernel, dim3((unsigned)((a.n + kRowsPerBlock - 1) / kRowsPerBlock)),
                     dim3(64 * kRowsPerBlock), 0, s, a, W);
  return hipGetLastError();
}

}  // namespace frecsys_hip
