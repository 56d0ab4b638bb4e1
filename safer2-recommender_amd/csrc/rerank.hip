// rerank.hip -- scores of caller-supplied (row, item) pairs and the ranking
// of caller-supplied per-row candidate lists on gfx950: the kernels behind
// frecsys_score_pairs and frecsys_rank_candidates.  The opposite regime from
// recommend.hip's scan: one Dp * 4-byte item row is gathered per 2 d flops, so
// the kernels are built around the gather, and the arithmetic is VALU.
//
//   rerank_history_kernel  rec_history_kernel's bitmap (recommend.hip keeps
//                          its kernel file-local): bit j of bitmap[row] = 1
//                          for every j of the row's CSR history;
//   score_pairs_kernel     one wave per 64 pairs.  Both operands' rows are
//                          gathered in 32-column slabs (8 lanes read the 128
//                          consecutive bytes of one row as float4, 8 rows per
//                          lane and slab), written k-major into LDS
//                          (s[kk * 65 + j], conflict-free both ways) and lane
//                          j runs the chain of pair j; the next slab's loads
//                          are in flight during the chain;
//   rank_cand_kernel       one workgroup of 256 per query row.  The row of X
//                          stays in LDS; the list is swept in chunks of 256
//                          candidates, gathered and staged like the pairs'
//                          item rows (ys[kk * 257 + j]), lane j scores
//                          candidate j of the chunk.  An eligible candidate
//                          (mask bit and not history bit) whose key is not
//                          below the row's threshold is appended as the
//                          project's candidate word (score_key << 32 | ~id) to
//                          a 2048-word buffer in LDS; before a chunk that
//                          might not fit, and at the end, the buffer is sorted
//                          by rec_merge_kernel's bitonic network, adjacent
//                          equal words collapse to one, and the best k stay.
//
// Score definition (both kernels): acc = fmaf(y[c], x[c], acc) for
// c = 0 .. Dp-1 ascending from +0 -- one lane, one serial chain, whatever the
// pair's position, chunk, workgroup or batch.  A chain from +0 never yields
// -0 (a sum is -0 only when both terms are), and the zero pad columns add +0,
// so the loops stop at Dp.
//
// Distinct ids: the ranking is over the DISTINCT ids of a list.  The same id
// has the same score (the chain does not depend on the position), hence the
// same word; after a sort equal words are adjacent and collapse, also when
// the repeats lay in different chunks (the kept copy meets the later one in
// the next sort).
//
// Threshold: set only when a sort leaves >= k distinct words, to the key of
// the k-th; a later candidate is appended when key >= threshold.  NOT the
// scan's strict rule: a caller's list is in no id order, so a later candidate
// that ties the k-th key may have a smaller id and beat it.  A candidate with
// a smaller key than k distinct candidates can never be listed: exact.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;

constexpr int CH = 256;            // candidates per chunk = threads of the rank workgroup
constexpr int KS = 32;             // columns per staged slab
constexpr int kRankSlots = 2048;   // candidate words in LDS: >= 1024 + CH

__global__ void __launch_bounds__(64)
    rerank_history_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
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

// Columns col0 + 4 q .. + 3 of the 8 rows at element offsets off[i] of table
// T into registers.  Unconditional loads (8 in flight): a slot without a row
// carries offset 0 (row 0 exists) and a float4 beyond the Dp columns (Dp = 8,
// 16) reads columns 0 .. 3 instead -- neither is ever read back from LDS.
__device__ __forceinline__ void slab_load(const float* __restrict__ T, const int64_t (&off)[8],
                                          int col0, int Dp, int q, f32x4v (&r)[8]) {
  const int col = col0 + 4 * q < Dp ? col0 + 4 * q : 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = *reinterpret_cast<const f32x4v*>(T + off[i] + col);
}

// ... and into the k-major LDS slab of NT rows: s[kk * (NT + 1) + j], row
// j = jb + (NT / 8) i.  A half-wave writes 8 q x 4 jb: 32 distinct banks.
template <int NT>
__device__ __forceinline__ void slab_store(float* s, int jb, int q, const f32x4v (&r)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = jb + (NT / 8) * i;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[(4 * q + e) * (NT + 1) + j] = r[i][e];
  }
}

__global__ void __launch_bounds__(64, 3) score_pairs_kernel(ScorePairsArgs a) {
  __shared__ float xs[KS * 65];
  __shared__ float ys[KS * 65];
  const int lane = threadIdx.x, q = lane & 7, jb = lane >> 3;
  const int64_t base = (int64_t)blockIdx.x * 64;
  const int Dp = a.Dp;
  int64_t offx[8], offy[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t p = base + jb + 8 * i;
    offx[i] = p < a.n ? a.rows[p] * Dp : 0;
    offy[i] = p < a.n ? (int64_t)a.items[p] * Dp : 0;
  }
  f32x4v px[8], py[8];
  slab_load(a.X, offx, 0, Dp, q, px);
  slab_load(a.Y, offy, 0, Dp, q, py);
  const int NC = (Dp + KS - 1) / KS;
  float acc = 0.0f;
  for (int c = 0; c < NC; ++c) {
    wave_lds_sync();  // the last slab's chain has read xs / ys
    slab_store<64>(xs, jb, q, px);
    slab_store<64>(ys, jb, q, py);
    wave_lds_sync();
    if (c + 1 < NC) {
      slab_load(a.X, offx, KS * (c + 1), Dp, q, px);
      slab_load(a.Y, offy, KS * (c + 1), Dp, q, py);
    }
    const int kmax = Dp - KS * c < KS ? Dp - KS * c : KS;
#pragma unroll 4
    for (int kk = 0; kk < kmax; ++kk) acc = fmaf(ys[kk * 65 + lane], xs[kk * 65 + lane], acc);
  }
  if (base + lane < a.n) a.out[base + lane] = acc;
}

// The `nn` words of wb sorted (descending), equal neighbours collapsed, the
// best min(distinct, k) left in wb[0 ..).  Returns that count; *tkey = the key
// of the k-th when there are k.  All 256 threads; scan: 4 ints of LDS.
__device__ __forceinline__ int sort_distinct(u64* wb, int nn, int k, int tid, int* scan,
                                             uint32_t* tkey) {
  int P = 256;
  while (P < nn) P <<= 1;  // <= kRankSlots
  for (int i = nn + tid; i < P; i += 256) wb[i] = 0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int p = tid; p < (P >> 1); p += 256) {
        const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        const int j = i | stride;
        const bool up = (i & size) == 0;
        const u64 x = wb[i], y = wb[j];
        if (up ? x < y : x > y) {
          wb[i] = y;
          wb[j] = x;
        }
      }
      __syncthreads();
    }
  }
  // thread t owns the E = P / 256 consecutive words from t E on
  const int E = P >> 8, i0 = tid * E;
  u64 v[kRankSlots / 256];
  u64 prev = i0 > 0 ? wb[i0 - 1] : 0ull;
  unsigned flags = 0;
  int mine = 0;
#pragma unroll
  for (int e = 0; e < kRankSlots / 256; ++e) {
    v[e] = 0ull;
    if (e < E) {
      v[e] = wb[i0 + e];
      if (v[e] != 0ull && v[e] != prev) {
        flags |= 1u << e;
        ++mine;
      }
      prev = v[e];
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) scan[wave] = incl;
  __syncthreads();  // every word read, the wave totals written
  int pos = incl - mine, total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) pos += scan[w];
    total += scan[w];
  }
#pragma unroll
  for (int e = 0; e < kRankSlots / 256; ++e) {
    if ((flags >> e) & 1u) {
      if (pos < k) wb[pos] = v[e];
      ++pos;
    }
  }
  __syncthreads();
  if (total >= k) *tkey = (uint32_t)(wb[k - 1] >> 32);
  return total < k ? total : k;
}

__global__ void __launch_bounds__(256, 3) rank_cand_kernel(RankCandArgs a, int64_t W) {
  __shared__ u64 wb[kRankSlots];
  __shared__ float ys[KS * (CH + 1)];
  __shared__ __attribute__((aligned(16))) float xs[1024];
  __shared__ int scan[4];
  __shared__ int cnt_s;
  const int tid = threadIdx.x, lane = tid & 63, q = tid & 7, jb = tid >> 3;
  const int64_t row = blockIdx.x;
  const int64_t xr = a.qrows ? a.qrows[a.r0 + row] : a.r0 + row;
  const int Dp = a.Dp, k = a.k;
  const int64_t p0 = a.cand_ptr[a.r0 + row] - a.cand_base;
  const int64_t len = a.cand_ptr[a.r0 + row + 1] - a.cand_base - p0;
  const int32_t* __restrict__ list = a.cand + p0;
  for (int c = tid; c < Dp; c += 256) xs[c] = a.X[xr * Dp + c];
  if (tid == 0) cnt_s = 0;
  uint32_t tkey = 0;  // a candidate passes with key >= tkey (0: no threshold yet); uniform
  int cnt = 0;        // words in wb between chunks; uniform
  const int NC = (Dp + KS - 1) / KS;
  const int64_t nchunks = (len + CH - 1) / CH;
  int64_t off[8];
  f32x4v pre[8];
  if (nchunks > 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t p = jb + 32 * i;
      off[i] = p < len ? (int64_t)list[p] * Dp : 0;
    }
    slab_load(a.Y, off, 0, Dp, q, pre);
  }
  for (int64_t chunk = 0; chunk < nchunks; ++chunk) {
    float acc = 0.0f;
    for (int c = 0; c < NC; ++c) {
      __syncthreads();  // the last slab's chains (and xs, cnt_s, a sort) are done
      slab_store<CH>(ys, jb, q, pre);
      __syncthreads();
      if (c + 1 < NC) {
        slab_load(a.Y, off, KS * (c + 1), Dp, q, pre);
      } else if (chunk + 1 < nchunks) {  // the next chunk's first slab
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int64_t p = (chunk + 1) * CH + jb + 32 * i;
          off[i] = p < len ? (int64_t)list[p] * Dp : 0;
        }
        slab_load(a.Y, off, 0, Dp, q, pre);
      }
      const int kmax = Dp - KS * c < KS ? Dp - KS * c : KS;
      const float* xc = xs + KS * c;
#pragma unroll 4
      for (int kk = 0; kk < kmax; ++kk) acc = fmaf(ys[kk * (CH + 1) + tid], xc[kk], acc);
    }
    // append: eligible, and not below the threshold
    const int64_t p = chunk * CH + tid;
    bool keep = false;
    u64 word = 0ull;
    if (p < len) {
      const uint32_t id = (uint32_t)list[p];
      const uint32_t key = score_key(acc);
      bool el = (a.maskw[id >> 5] >> (id & 31)) & 1u;
      if (el && a.bitmap) el = !((a.bitmap[row * W + (id >> 5)] >> (id & 31)) & 1u);
      keep = el && key >= tkey;
      word = ((u64)key << 32) | (uint32_t)~id;
    }
    const u64 bal = __ballot(keep);
    if (bal) {  // wave-uniform: one LDS atomic per wave
      int slot = 0;
      if (lane == __ffsll((long long)bal) - 1) slot = atomicAdd(&cnt_s, __popcll(bal));
      slot = __shfl(slot, __ffsll((long long)bal) - 1);
      slot += __popcll(bal & ((1ull << lane) - 1ull));
      // slot < kRankSlots always: a chunk starts with cnt <= kRankSlots - CH
      if (keep && slot < kRankSlots) wb[slot] = word;
    }
    __syncthreads();
    cnt = cnt_s;
    if (cnt > kRankSlots - CH && chunk + 1 < nchunks) {  // uniform
      cnt = sort_distinct(wb, cnt, k, tid, scan, &tkey);
      if (tid == 0) cnt_s = cnt;
    }
  }
  __syncthreads();
  const int keep_n = sort_distinct(wb, cnt, k, tid, scan, &tkey);
  for (int i = tid; i < k; i += 256) {
    const u64 v = i < keep_n ? wb[i] : 0ull;
    a.out_items[row * k + i] = v ? (int32_t)~(uint32_t)v : -1;
    if (a.out_scores) a.out_scores[row * k + i] = v ? score_unkey((uint32_t)(v >> 32)) : -FLT_MAX;
  }
}

}  // namespace

int rank_cand_chunk() { return CH; }
int rank_cand_slots() { return kRankSlots; }

hipError_t launch_score_pairs(const ScorePairsArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (!a.X || !a.Y || !a.rows || !a.items || !a.out || a.Dp < 1 || a.Dp > 1024 || (a.Dp & 7))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(score_pairs_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rank_candidates(const RankCandArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.k < 1 || a.k > 1024 || a.m < 1 || !a.X || !a.Y || !a.maskw || !a.cand_ptr || !a.cand ||
      !a.out_items || a.Dp < 1 || a.Dp > 1024 || (a.Dp & 7))
    return hipErrorInvalidValue;
  const int64_t W = recommend_words(a.m);
  if (a.bitmap) {
    if (!a.row_ptr || !a.col) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.bitmap, 0, sizeof(uint32_t) * (size_t)a.n * (size_t)W, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rerank_history_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a.row_ptr,
                       a.col, a.qrows, a.r0, a.m, W, a.bitmap);
  }
  hipLaunchKernelGGL(rank_cand_kernel, dim3((unsigned)a.n), dim3(256), 0, s, a, W);
  return hipGetLastError();
}

}  // namespace frecsys_hip
