// audience.hip -- the thin-query scan behind frecsys_audience: a few query
// rows (items) against the largest table the model has (users).  The fused
// scan of recommend.hip is a 64-row x 128-item MFMA tile: with n <= 64 queries
// it launches one row block, at most 8192 / k workgroups, and 1 / 64 of every
// tile is useful per query present.  This path is shaped the other way round:
//
//   thin_scan_kernel   grid (passes) x (splits).  A workgroup holds the QT
//                      queries of its pass (scalar loads: a query value is the
//                      SGPR operand of its rows' FMAs) and sweeps the CR-row
//                      chunks of its split in ascending id.  A chunk comes in
//                      32-column slabs: 16-B loads, 8 lanes per 128-B row
//                      segment, staged through LDS one slab ahead in
//                      registers.  Thread t then owns row t % CR of the chunk
//                      and the queries of half t / CR (wave-uniform), and runs
//                      QT / 2 independent chains acc = fmaf(X[q][c], Y[row][c],
//                      acc), c ascending from +0 -- recommend.hip's score,
//                      frecsys_score_pairs', bit for bit.  Every row of Y is
//                      read from memory once per pass.
//                      Candidates are recommend.hip's words (score_key << 32 |
//                      ~id) in a buffer per (query, split) of `slots` words;
//                      a buffer that the next chunk could overflow is cut to
//                      its best k by one wave (bitonic sort in the LDS the slab
//                      had), and the threshold moves only there;
//   aud_history_kernel rec_history_kernel's bits, a query's CSR row cut over 32
//                      workgroups (a popular item's row has tens of thousands
//                      of entries);
//   aud_reduce_kernel  grid (queries) x (groups): the k best words of a group
//                      of sorted lists, sorted, by pairwise bitonic merges.
//                      The words of a query are distinct and totally ordered,
//                      so "the k largest of a set" does not depend on the
//                      grouping, the rounds or the splits;
//   rec_merge_kernel   (recommend.hip) on the one list left: ids and scores
//                      out, -1 / -FLT_MAX beyond the eligible count.
//
// Tie invariant (recommend.hip's): a (query, split) pair is swept once, by one
// workgroup, chunk after chunk in ascending id, and its threshold is set only
// between two chunks, to the key of the k-th best word so far.  A candidate of
// a later chunk has a larger id than every word kept, so at equal key its word
// is smaller than the k-th best: key > threshold, strictly, loses nothing.
// Inside a chunk the appends are unordered, and the threshold does not move.
//
// Offsets into X and Y are 64-bit (row * Dp as int64_t): 2M x 1024 floats are
// 2^31 elements.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;
typedef const __attribute__((address_space(4))) float* cfloat_p;
typedef const __attribute__((address_space(4))) int64_t* cint64_p;

constexpr int QT = 8;               // queries held on chip per pass, half of them per thread
constexpr int CR = 128;             // rows per chunk
constexpr int KS = 32;              // columns per slab
constexpr int LDW = KS + 1;         // slab row stride in LDS: lanes over rows, conflict-free
constexpr int NP = CR * KS / 1024;  // 16-B pieces of a slab per thread
constexpr int kSortWords = 2048;    // the slab's LDS as sort slices: 16,896 B >= 16 KiB
constexpr int kMergeSlots = 8192;   // rec_merge_kernel's and aud_reduce_kernel's LDS words

// The `nn` (<= cap) words of buffer g sorted (descending) by one wave in its
// LDS slice sb; the best min(nn, k) written back, in order.  Returns that
// count; *kth = the k-th best word when nn >= k.  (recommend.hip's
// compact_row with the slot count at run time.)
__device__ __forceinline__ int compact_list(u64* __restrict__ g, u64* sb, int nn, int cap, int k,
                                            int lane, u64* kth) {
  if (nn > cap) nn = cap;  // never: a query enters a chunk with at most cap - CR words
  int P = 64;
  while (P < nn) P <<= 1;
  for (int i = lane; i < P; i += 64) sb[i] = i < nn ? g[i] : 0ull;
  wave_lds_sync();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int p = lane; p < (P >> 1); p += 64) {
        const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        const int j = i | stride;
        const bool up = (i & size) == 0;
        const u64 a = sb[i], b = sb[j];
        if (up ? a < b : a > b) {
          sb[i] = b;
          sb[j] = a;
        }
      }
      wave_lds_sync();
    }
  }
  const int keep = nn < k ? nn : k;
  for (int i = lane; i < keep; i += 64) g[i] = sb[i];
  if (nn >= k) *kth = sb[k - 1];
  wave_lds_sync();
  return keep;
}

// Slab `c` of the chunk at row0 into registers: piece j of thread t is the
// 16 B at columns 32 c + 4 (t & 7) of row ((j * 256 + t) >> 3) -- 8 lanes per
// 128-B row segment.  Rows past m and columns past Dp read as zero.
__device__ __forceinline__ void slab_load(const float* __restrict__ Y, int64_t m, int Dp,
                                          int64_t row0, int c, int tid, f32x4v (&pre)[NP]) {
  const int col = KS * c + 4 * (tid & 7);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int64_t row = row0 + ((j * 256 + tid) >> 3);
    pre[j] = (row < m && col < Dp) ? *reinterpret_cast<const f32x4v*>(Y + row * Dp + col)
                                   : f32x4v{0.f, 0.f, 0.f, 0.f};
  }
}

// 8 waves per SIMD: 8 workgroups of 17 KB per CU, so that the scalar loads of
// one wave's queries wait behind the FMAs of seven others.
template <int QTN>
__global__ void __launch_bounds__(256, 8)
    thin_scan_kernel(AudienceArgs a, int64_t W, int slots) {
  constexpr int QHN = QTN / 2;
  __shared__ __attribute__((aligned(16))) float slab[CR * LDW];
  __shared__ uint32_t tkey[QTN];  // a candidate passes with key >= tkey (0: no threshold yet)
  __shared__ int cnt[QTN];
  static_assert(sizeof(float) * CR * LDW >= sizeof(u64) * kSortWords, "sort slices in the slab");
  u64* const sortbuf = reinterpret_cast<u64*>(slab);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = wave >> 1;                    // the thread's queries: half * QHN .. + QHN - 1
  const int rl = tid & (CR - 1);                 // its row in the chunk
  const int64_t q0 = (int64_t)blockIdx.x * QTN;  // the pass's first query in the batch
  const int split = blockIdx.y, splits = a.splits;
  const int nq = (int)(a.n - q0 < QTN ? a.n - q0 : QTN);
  const int64_t nchunks = (a.m + CR - 1) / CR;
  const int64_t c0 = split * nchunks / splits, c1 = (split + 1) * nchunks / splits;
  const int Dp = a.Dp, k = a.k;
  const int NC = (Dp + KS - 1) / KS;
  const int nsort = kSortWords / slots < 4 ? kSortWords / slots : 4;  // waves that sort at once

  // the queries: uniform addresses in the constant address space (the tables
  // are not written while a ranking call runs), so the loads are scalar
  const cfloat_p Xc = (cfloat_p)a.X;
  const cint64_p qrc = (cint64_p)a.qrows;
  int64_t qoff[QHN];
#pragma unroll
  for (int i = 0; i < QHN; ++i) {
    const int qq = half * QHN + i;
    const int64_t qi = a.r0 + q0 + (qq < nq ? qq : 0);  // spare chains repeat the first query
    qoff[i] = (qrc ? qrc[qi] : qi) * Dp;
  }
  if (tid < QTN) {
    cnt[tid] = 0;
    tkey[tid] = 0u;
  }
  __syncthreads();

  f32x4v pre[NP];
  for (int64_t chunk = c0; chunk < c1; ++chunk) {
    const int64_t row0 = chunk * CR;
    slab_load(a.Y, a.m, Dp, row0, 0, tid, pre);
    // a buffer that this chunk could overflow is cut to its best k (the slab's
    // LDS is free: every wave is past the barrier behind the last appends)
    if (wave < nsort) {
      for (int i = wave; i < nq; i += nsort) {
        const int nn = cnt[i];
        if (nn > slots - CR) {  // wave-uniform
          u64 kth = 0ull;
          const int keep = compact_list(a.cand + ((q0 + i) * splits + split) * (int64_t)slots,
                                        sortbuf + wave * slots, nn, slots, k, lane, &kth);
          if (lane == 0) {
            cnt[i] = keep;
            if (nn >= k) tkey[i] = (uint32_t)(kth >> 32) + 1u;
          }
        }
      }
    }
    float acc[QHN];
#pragma unroll
    for (int i = 0; i < QHN; ++i) acc[i] = 0.0f;
    for (int c = 0; c < NC; ++c) {
      __syncthreads();  // the last slab's reads, or the sorts, are done
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        float* d = slab + ((j * 256 + tid) >> 3) * LDW + 4 * (tid & 7);
        d[0] = pre[j][0];
        d[1] = pre[j][1];
        d[2] = pre[j][2];
        d[3] = pre[j][3];
      }
      __syncthreads();
      if (c + 1 < NC) slab_load(a.Y, a.m, Dp, row0, c + 1, tid, pre);  // in flight over the FMAs
      const int kw = Dp - KS * c < KS ? Dp - KS * c : KS;  // a multiple of 8
      const float* yr = slab + rl * LDW;
      for (int kb = 0; kb < kw; kb += 8) {
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = yr[kb + j];
#pragma unroll
        for (int i = 0; i < QHN; ++i) {
          float q[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) q[j] = Xc[qoff[i] + KS * c + kb + j];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i] = __builtin_fmaf(q[j], y[j], acc[i]);
        }
      }
    }
    // append: the thread's row against its queries' thresholds and histories
    {
      const int64_t id = row0 + rl;
      const bool ok = id < a.m && ((a.maskw[id >> 5] >> (id & 31)) & 1u);
#pragma unroll
      for (int i = 0; i < QHN; ++i) {
        const int qq = half * QHN + i;
        if (qq < nq && ok) {
          const uint32_t key = score_key(acc[i]);
          bool take = key >= tkey[qq];
          if (take && a.bitmap) take = !((a.bitmap[(q0 + qq) * W + (id >> 5)] >> (id & 31)) & 1u);
          if (take) {
            const int slot = atomicAdd(&cnt[qq], 1);
            // slot < slots always: a query enters a chunk with cnt <= slots - CR
            if (slot < slots)
              a.cand[((q0 + qq) * splits + split) * (int64_t)slots + slot] =
                  ((u64)key << 32) | ~(uint32_t)id;
          }
        }
      }
    }
    __syncthreads();
  }
  if (wave < nsort) {
    for (int i = wave; i < nq; i += nsort) {
      u64 kth = 0ull;
      const int keep = compact_list(a.cand + ((q0 + i) * splits + split) * (int64_t)slots,
                                    sortbuf + wave * slots, cnt[i], slots, k, lane, &kth);
      if (lane == 0) a.counts[(q0 + i) * splits + split] = keep;
    }
  }
}

// The k best words of lists [g G, min(L, (g + 1) G)) of query blockIdx.x,
// sorted, to list g = blockIdx.y of `out` (k words apart).  Every list comes in
// sorted (descending), so no sort is needed: the lists, padded with zeros to
// kp words (kp: k rounded up to a power of two, G kp = kMergeSlots), are
// merged in pairs, level by level.  A level keeps max(a[i], b[kp - 1 - i]) in
// a's place -- the kp largest of the pair as a bitonic sequence -- and sorts
// it with the log2(kp) passes of a bitonic merge.  (A full bitonic sort of the
// group's words, the first build's reduce, took most of a 0.3 ms call.)
__global__ void __launch_bounds__(256)
    aud_reduce_kernel(const u64* __restrict__ in, const int32_t* __restrict__ cin, int L,
                      int64_t stride, int G, int kp, int k, u64* __restrict__ out,
                      int32_t* __restrict__ cout) {
  __shared__ u64 mb[kMergeSlots];
  const int tid = threadIdx.x, g = blockIdx.y, Lout = gridDim.y;
  const int64_t row = blockIdx.x;
  const int s0 = g * G;
  int total = 0;
  for (int j = 0; j < G; ++j) {
    int c = 0;
    if (s0 + j < L) {
      c = cin[row * L + s0 + j];
      if (c > k) c = k;
    }
    const u64* src = in + (row * L + s0 + j) * stride;  // read below c only
    for (int i = tid; i < kp; i += 256) mb[j * kp + i] = i < c ? src[i] : 0ull;
    total += c;
  }
  __syncthreads();
  const int hk = kp >> 1;
  for (int st = 1; st < G; st <<= 1) {  // lists j with j % (2 st) == 0 survive the level
    const int pairs = G / (2 * st);
    for (int e = tid; e < pairs * kp; e += 256) {
      const int pr = e / kp, i = e - pr * kp;
      u64* la = mb + (2 * pr * st) * kp;
      const u64 x = la[i], y = la[st * kp + kp - 1 - i];
      if (y > x) la[i] = y;
    }
    __syncthreads();
    for (int d = hk; d > 0; d >>= 1) {
      for (int e = tid; e < pairs * hk; e += 256) {
        const int pr = e / hk, j = e - pr * hk;
        const int i = ((j & ~(d - 1)) << 1) | (j & (d - 1));
        u64* la = mb + (2 * pr * st) * kp;
        const u64 x = la[i], y = la[i | d];
        if (x < y) {
          la[i] = y;
          la[i | d] = x;
        }
      }
      __syncthreads();
    }
  }
  const int keep = total < k ? total : k;
  u64* dst = out + (row * Lout + g) * (int64_t)k;
  for (int i = tid; i < keep; i += 256) dst[i] = mb[i];
  if (tid == 0) cout[row * Lout + g] = keep;
}

// rec_history_kernel's bits with kHistParts workgroups per query: the ITEM-side
// row of a popular item has tens of thousands of entries, which one wave
// takes 0.7 ms to set (measured: the synthetic ML-20M head item, 64,000 users).
constexpr int kHistParts = 32;
__global__ void __launch_bounds__(256)
    aud_history_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                       const int64_t* __restrict__ qrows, int64_t r0, int64_t m, int64_t W,
                       uint32_t* __restrict__ bitmap) {
  const int64_t u = blockIdx.x;
  const int64_t e = qrows ? qrows[r0 + u] : r0 + u;
  const int64_t p0 = row_ptr[e], len = row_ptr[e + 1] - p0;
  const int64_t a = p0 + len * blockIdx.y / kHistParts, b = p0 + len * (blockIdx.y + 1) / kHistParts;
  for (int64_t p = a + threadIdx.x; p < b; p += 256) {
    const int64_t j = col[p];
    if (j >= 0 && j < m) atomicOr(&bitmap[u * W + (j >> 5)], 1u << (j & 31));
  }
}

}  // namespace

int audience_queries_per_pass() { return QT; }
int audience_chunk_rows() { return CR; }

int audience_slots(int k) {
  int s = 256;
  while (s < k + CR) s <<= 1;
  return s;
}

// k rounded up to a power of two, 64 at least: the length of a list in the
// reduce kernel's LDS.
static int reduce_kp(int k) {
  int kp = 64;
  while (kp < k) kp <<= 1;
  return kp;
}

int audience_group(int k) { return kMergeSlots / reduce_kp(k); }

int audience_reduce_lists(int splits, int k) {
  const int G = audience_group(k);
  return splits > 1 ? (splits + G - 1) / G : 0;
}

int audience_merge_rounds(int splits, int k) {
  const int G = audience_group(k);
  int rounds = 1;
  for (int L = splits; L > 1; L = (L + G - 1) / G) ++rounds;
  return rounds;
}

hipError_t launch_audience_thin(const AudienceArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const int64_t nchunks = (a.m + CR - 1) / CR;
  if (a.k < 1 || a.k > 1024 || a.m < 1 || a.splits < 1 || a.splits > nchunks || a.splits > 65535 ||
      (a.Dp & 7) || !a.X || !a.Y || !a.maskw || !a.cand || !a.counts || !a.out_items ||
      (audience_reduce_lists(a.splits, a.k) > 0 && (!a.red || !a.red_counts)))
    return hipErrorInvalidValue;
  const int64_t W = recommend_words(a.m);
  if (a.bitmap) {
    if (!a.row_ptr || !a.col) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.bitmap, 0, sizeof(uint32_t) * (size_t)a.n * (size_t)W, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(aud_history_kernel, dim3((unsigned)a.n, kHistParts), dim3(256), 0, s,
                       a.row_ptr, a.col, a.qrows, a.r0, a.m, W, a.bitmap);
  }
  const int slots = audience_slots(a.k);
  const unsigned passes = (unsigned)((a.n + QT - 1) / QT);
  hipLaunchKernelGGL((thin_scan_kernel<QT>), dim3(passes, (unsigned)a.splits), dim3(256), 0, s, a,
                     W, slots);
  // rounds: the lists of a query, `stride` words apart, between the two regions,
  // until one is left for rec_merge_kernel to write out
  const int G = audience_group(a.k), kp = reduce_kp(a.k);
  const u64* in = a.cand;
  const int32_t* cin = a.counts;
  int64_t stride = slots;
  int L = a.splits;
  bool to_red = true;
  while (L > 1) {
    const int Lout = (L + G - 1) / G;
    u64* out = to_red ? a.red : a.cand;
    int32_t* cout = to_red ? a.red_counts : a.counts;
    hipLaunchKernelGGL(aud_reduce_kernel, dim3((unsigned)a.n, (unsigned)Lout), dim3(256), 0, s, in,
                       cin, L, stride, G, kp, a.k, out, cout);
    in = out;
    cin = cout;
    stride = a.k;
    L = Lout;
    to_red = !to_red;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  RecommendArgs r{};
  r.n = a.n;
  r.k = a.k;
  r.splits = L;
  r.cand = const_cast<u64*>(in);
  r.counts = const_cast<int32_t*>(cin);
  r.out_items = a.out_items;
  r.out_scores = a.out_scores;
  return launch_recommend_merge(r, stride, s);
}

}  // namespace frecsys_hip
