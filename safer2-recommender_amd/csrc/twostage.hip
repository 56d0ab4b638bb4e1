// twostage.hip -- retrieve-then-rank on gfx950: the kernels behind
// frecsys_recommend_two_stage (the definitions are in include/frecsys_hip.h).
//
//   ts_convert_kernel  one workgroup per 128-item tile: the bf16 image of the
//                      item table in the scan's granule order (kernels.h
//                      two_stage_image_bytes), per-row norms in double, the
//                      largest norm and the count of subnormal bf16 values;
//   ts_scan_kernel     rec_scan_kernel's grid, tiles, eligibility words,
//                      threshold rule, appends and compact_row cuts, but the
//                      64 x 128 scores of a tile come from
//                      v_mfma_f32_32x32x16_bf16: the workgroup's 64 query rows
//                      are rounded to bf16 once and stay in LDS for the whole
//                      sweep ([granule][row], 32 KB at Dp = 256, 128 KB at
//                      1024), and the tile's item granules are streamed from
//                      the image in k-slabs through two LDS buffers, the next
//                      slab's loads in flight during a slab's MFMAs;
//   ts_select_kernel   one workgroup per query row: the pool's items re-scored
//                      by rank_cand_kernel's gather and chain (recommend.hip's
//                      score, bit for bit), the k best by one bitonic sort of
//                      the pool's words, and the row's certificate.
//
// Stage-1 score: acc = mfma(y^[k0..k0+15], x^[k0..k0+15], acc) for k0 = 0, 16,
// ... ascending from +0, operands swapped as in rec_scan_kernel (items are the
// MFMA's A rows, query rows its B columns, so a lane holds scores of ONE query
// row).  The order of the k-steps is fixed, so a (row, item) pair has the same
// accumulator bits in every tile, split, batch and grid.  The threshold
// invariant is rec_scan_kernel's: ids ascend along the sweep, so the strict
// test key > threshold is exact for the keys of THIS score.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "common.h"
#include "kernels.h"
#include "scan_words.h"

namespace frecsys_hip {

namespace {

typedef unsigned long long u64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int RT = 64;   // query rows per workgroup
constexpr int IT = 128;  // items per tile

// 8 consecutive columns as one bf16 granule; *sub counts the subnormal ones.
__device__ __forceinline__ u32x4 pack_granule(const float (&v)[8], int* sub) {
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    h[j] = bf16_round_bits(__float_as_uint(v[j]));
    if (sub && bf16_subnormal(h[j])) ++*sub;
  }
  u32x4 g;
#pragma unroll
  for (int j = 0; j < 4; ++j) g[j] = h[2 * j] | (h[2 * j + 1] << 16);
  return g;
}

// Columns 8 g .. 8 g + 7 of a row of ld Dp (zero beyond Dp, or without a row).
__device__ __forceinline__ void load_granule(const float* __restrict__ row, int g, int Dp,
                                             float (&v)[8]) {
  if (row && 8 * g < Dp) {
    const f32x4v a = *reinterpret_cast<const f32x4v*>(row + 8 * g);
    const f32x4v b = *reinterpret_cast<const f32x4v*>(row + 8 * g + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a[j], v[4 + j] = b[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0f;
  }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// A wave per item row, a lane per granule: coalesced reads of the fp32 row.
__global__ void __launch_bounds__(256)
    ts_convert_kernel(const float* __restrict__ T, int64_t m, int Dp, int Dh,
                      u32x4* __restrict__ image, double* __restrict__ norms,
                      u64* __restrict__ stats) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int G = Dh >> 3;
  for (int j = wave; j < IT; j += 4) {
    const int64_t it = tile * IT + j;
    const float* row = it < m ? T + it * Dp : nullptr;
    double sq = 0.0;
    int sub = 0;
    for (int g = lane; g < G; g += 64) {
      float v[8];
      load_granule(row, g, Dp, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) sq += (double)v[e] * (double)v[e];
      image[(tile * G + g) * IT + j] = pack_granule(v, &sub);
    }
    if (it >= m) continue;  // wave-uniform
    sq = wave_sum(sq);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sub += __shfl_xor(sub, o);
    if (lane == 0) {
      const double nr = sqrt(sq);
      norms[it] = nr;
      // non-negative doubles order as their bits; a NaN is the largest
      atomicMax(&stats[0], nr != nr ? 0x7ff8000000000000ull : (u64)__double_as_longlong(nr));
      if (sub) atomicAdd(&stats[1], (u64)sub);
    }
  }
}

// SG: granules (8 columns each) of a k-slab; two slab buffers of SG * IT
// granules.  The waves' sort slices share the slab buffers: a wave sorts only
// between the barrier that ends a tile's appends and the barrier before the
// next tile's first slab is stored, so NS = as many slices as the buffers hold
// (at most one per wave) sort at a time.
template <int CAP, int SG>
__global__ void __launch_bounds__(256) ts_scan_kernel(RecommendArgs a, const u32x4* __restrict__ img,
                                                      int64_t W, int Dh) {
  constexpr int kStageBytes = 2 * SG * IT * 16;
  constexpr int NS = kStageBytes / (CAP * 8) >= 4 ? 4 : kStageBytes / (CAP * 8);
  static_assert(NS >= 1, "a sort slice must fit the slab buffers");
  constexpr int PF = SG / 2;  // granules a thread moves per slab
  extern __shared__ __attribute__((aligned(16))) char ts_lds[];
  u32x4* ys = reinterpret_cast<u32x4*>(ts_lds);                // [2][SG][IT]
  u64* sortbuf = reinterpret_cast<u64*>(ts_lds);               // [NS][CAP]
  u32x4* xq = reinterpret_cast<u32x4*>(ts_lds + kStageBytes);  // [Dh / 8][RT]
  __shared__ uint32_t tkey[RT];  // a candidate passes with key >= tkey (0: no threshold yet)
  __shared__ int cnt[RT];
  __shared__ uint32_t elig[RT * 4];
  __shared__ int64_t xrow[RT];
  __shared__ u64* cbase[RT];  // the row's candidate buffer of this split
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t base = (int64_t)blockIdx.x * RT;
  const int split = blockIdx.y, splits = a.splits;
  const int64_t ntiles = (a.m + IT - 1) / IT;
  const int64_t t0 = split * ntiles / splits, t1 = (split + 1) * ntiles / splits;
  const int Dp = a.Dp;
  const int R = wave & 1, Cs = (wave >> 1) * 2;
  const int G = Dh >> 3;              // granules per row: 2, or a multiple of 4
  const int gs = G < SG ? G : SG;     // granules per slab (even) ...
  const int NSL = (G + gs - 1) / gs;  // ... of the slabs of a tile, but in a shorter last one
  // (G = 12, 20, 28 at Dp = 96, 160, 224: a last slab of 4); the k-steps ascend through it
  const auto slab_granules = [&](int sl) { return G - sl * gs < gs ? G - sl * gs : gs; };
  if (tid < RT) {
    const int64_t row = base + tid;
    xrow[tid] = row < a.n ? (a.qrows ? a.qrows[a.r0 + row] : a.r0 + row) : -1;
    cnt[tid] = 0;
    cbase[tid] = a.cand + ((base + tid) * splits + split) * CAP;  // used for rows < n only
    tkey[tid] = row < a.n ? 0u : 0xffffffffu;
  }
  __syncthreads();
  // the query block, rounded once: lanes over the granules of a row
  for (int s = tid; s < RT * G; s += 256) {
    const int rr = s / G, g = s - rr * G;
    const int64_t xr = xrow[rr];
    float v[8];
    load_granule(xr >= 0 ? a.X + xr * Dp : nullptr, g, Dp, v);
    xq[g * RT + rr] = pack_granule(v, nullptr);
  }
  const int rl = 32 * R + lo;  // the lane's query row in the block
  u64* const mycand = a.cand + ((base + rl) * splits + split) * CAP;
  u32x4 pre[PF];
  auto load_slab = [&](int64_t tile, int sl) {
    const u32x4* src = img + (tile * G + (int64_t)sl * gs) * IT;  // its granules in a run
    const int cnt_g = slab_granules(sl) * IT;
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int idx = tid + 256 * i;
      if (idx < cnt_g) pre[i] = src[idx];
    }
  };
  auto store_slab = [&](int buf, int sl) {  // what load_slab(., sl) left in `pre`
    const int cnt_g = slab_granules(sl) * IT;
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int idx = tid + 256 * i;
      if (idx < cnt_g) ys[buf * SG * IT + idx] = pre[i];
    }
  };
  if (t0 < t1) load_slab(t0, 0);
  int buf = 0;
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
    }
    f32x16 acc[2] = {f32x16{0.f}, f32x16{0.f}};
    for (int sl = 0; sl < NSL; ++sl) {
      // buffer `buf` was last read two slabs ago: every wave has passed the
      // barrier of the slab between (or the one that closed the last tile)
      store_slab(buf, sl);
      __syncthreads();
      if (sl + 1 < NSL)
        load_slab(tile, sl + 1);
      else if (tile + 1 < t1)
        load_slab(tile + 1, 0);
      const u32x4* yb = ys + buf * SG * IT;
      const int gn = slab_granules(sl);
      for (int gg = 0; gg < gn; gg += 2) {  // one k-step: granules gg (hi = 0), gg + 1 (hi = 1)
        const bf16x8 xf = __builtin_bit_cast(bf16x8, xq[(sl * gs + gg + hi) * RT + rl]);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          // items as the MFMA's A rows, query rows as its B columns: the
          // accumulator holds S^T, a lane the scores of ONE query row
          const bf16x8 yf = __builtin_bit_cast(bf16x8, yb[(gg + hi) * IT + 32 * (Cs + t) + lo]);
          acc[t] = mfma_bf16(yf, xf, acc[t]);
        }
      }
      buf ^= 1;
    }
    // append: rec_scan_kernel's, word for word
    {
      const uint32_t tk = tkey[rl];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int C = Cs + t;
        const uint32_t ew = elig[rl * 4 + C];
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
    if (wave < NS) {
      for (int r = wave; r < RT; r += NS) {
        const int nn = cnt[r];
        if (nn > CAP - IT) {  // wave-uniform
          u64 kth = 0ull;
          const int keep = compact_row<CAP>(cbase[r], sortbuf + wave * CAP, nn, a.k, lane, &kth);
          if (lane == 0) {
            cnt[r] = keep;
            if (nn >= a.k) tkey[r] = (uint32_t)(kth >> 32) + 1u;
          }
        }
      }
    }
    __syncthreads();  // the sort slices are the slab buffers
  }
  __syncthreads();
  if (wave < NS) {
    for (int r = wave; r < RT; r += NS) {
      if (base + r >= a.n) continue;
      u64 kth = 0ull;
      const int keep = compact_row<CAP>(cbase[r], sortbuf + wave * CAP, cnt[r], a.k, lane, &kth);
      if (lane == 0) a.counts[(base + r) * splits + split] = keep;
    }
  }
}

// ---- stage 2 ----
constexpr int CH = 256;  // pool slots per chunk = threads of the select workgroup
constexpr int KS = 32;   // columns per staged slab
constexpr int kMaxPool = 1024;

// rank_cand_kernel's gather (rerank.hip keeps its copy file-local): columns
// col0 + 4 q .. + 3 of the 8 rows at element offsets off[i] into registers
// (unconditional loads: a slot without a row carries offset 0, and a float4
// beyond the Dp columns reads columns 0 .. 3 -- neither is read back) ...
__device__ __forceinline__ void slab_load(const float* __restrict__ T, const int64_t (&off)[8],
                                          int col0, int Dp, int q, f32x4v (&r)[8]) {
  const int col = col0 + 4 * q < Dp ? col0 + 4 * q : 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = *reinterpret_cast<const f32x4v*>(T + off[i] + col);
}
// ... and into the k-major LDS slab: s[kk * (CH + 1) + j], row j = jb + 32 i.
__device__ __forceinline__ void slab_store(float* s, int jb, int q, const f32x4v (&r)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = jb + (CH / 8) * i;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[(4 * q + e) * (CH + 1) + j] = r[i][e];
  }
}

__global__ void __launch_bounds__(256, 3) ts_select_kernel(TwoStageSelectArgs a) {
  __shared__ u64 wb[kMaxPool];
  __shared__ float ys[KS * (CH + 1)];
  __shared__ __attribute__((aligned(16))) float xs[1024];
  __shared__ double red[256];
  const int tid = threadIdx.x, q = tid & 7, jb = tid >> 3;
  const int64_t row = blockIdx.x;
  const int64_t xr = a.qrows ? a.qrows[a.r0 + row] : a.r0 + row;
  const int Dp = a.Dp, k = a.k, pool = a.pool;
  const int32_t* __restrict__ list = a.pool_items + row * pool;
  // the query row: into LDS, its squares summed in double (a fixed tree), and
  // whether one of its bf16 values is subnormal
  double sq = 0.0;
  int qsub = 0;
  for (int c = tid; c < Dp; c += 256) {
    const float v = a.X[xr * Dp + c];
    xs[c] = v;
    sq += (double)v * (double)v;
    qsub |= bf16_subnormal(bf16_round_bits(__float_as_uint(v))) ? 1 : 0;
  }
  red[tid] = sq;
  qsub = __syncthreads_or(qsub);  // also: xs and red are written
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double xnorm = sqrt(red[0]);
  const int NC = (Dp + KS - 1) / KS;
  const int nchunks = (pool + CH - 1) / CH;
  int fill = 0;
  int64_t off[8];
  f32x4v pre[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = jb + 32 * i;
    const int32_t id = p < pool ? list[p] : -1;
    off[i] = id >= 0 ? (int64_t)id * Dp : 0;
  }
  slab_load(a.Y, off, 0, Dp, q, pre);
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    float acc = 0.0f;
    for (int c = 0; c < NC; ++c) {
      __syncthreads();  // the last slab's chains are done
      slab_store(ys, jb, q, pre);
      __syncthreads();
      if (c + 1 < NC) {
        slab_load(a.Y, off, KS * (c + 1), Dp, q, pre);
      } else if (chunk + 1 < nchunks) {  // the next chunk's first slab
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int p = (chunk + 1) * CH + jb + 32 * i;
          const int32_t id = p < pool ? list[p] : -1;
          off[i] = id >= 0 ? (int64_t)id * Dp : 0;
        }
        slab_load(a.Y, off, 0, Dp, q, pre);
      }
      const int kmax = Dp - KS * c < KS ? Dp - KS * c : KS;
      const float* xc = xs + KS * c;
#pragma unroll 4
      for (int kk = 0; kk < kmax; ++kk) acc = fmaf(ys[kk * (CH + 1) + tid], xc[kk], acc);
    }
    const int p = chunk * CH + tid;
    const int32_t id = p < pool ? list[p] : -1;
    if (p < kMaxPool) wb[p] = id >= 0 ? ((u64)score_key(acc) << 32) | (uint32_t)~(uint32_t)id : 0ull;
    fill += __syncthreads_count(id >= 0);
  }
  // the words sorted descending (rec_merge_kernel's network); empty slots last
  int P = 2;
  while (P < pool) P <<= 1;  // <= kMaxPool
  for (int i = nchunks * CH + tid; i < P; i += 256) wb[i] = 0ull;
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
  for (int i = tid; i < k; i += 256) {
    const u64 v = i < fill ? wb[i] : 0ull;
    a.out_items[row * k + i] = v ? (int32_t)~(uint32_t)v : -1;
    a.out_scores[row * k + i] = v ? score_unkey((uint32_t)(v >> 32)) : -FLT_MAX;
  }
  if (tid == 0) {
    // (a) a pool that is not full holds every eligible item; (b) no item
    // outside a full pool can reach the k-th exact score.  No contraction:
    // the bound is frecsys_two_stage_bound's arithmetic.
    bool ok = a.stats[1] == 0ull && !qsub;
    if (ok && fill >= pool) {
      const double sk = (double)score_unkey((uint32_t)(wb[k - 1] >> 32));
      const double sp = (double)a.pool_scores[row * pool + pool - 1];
      const double nmax = __longlong_as_double((long long)a.stats[0]);
      const double B = __dmul_rn(__dmul_rn(two_stage_c(Dp), xnorm), nmax);
      ok = fill >= k && isfinite(sk) && isfinite(sp) && isfinite(B) && sk > __dadd_rn(sp, B);
    }
    a.certified[row] = ok ? 1 : 0;
  }
}

template <int CAP, int SG>
hipError_t launch_scan(const RecommendArgs& a, const void* image, int64_t W, int Dh,
                       hipStream_t s) {
  static bool attr = false;
  if (!attr) {  // room for the widest query block, 128 KB
    hipError_t err = hipFuncSetAttribute((const void*)ts_scan_kernel<CAP, SG>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         2 * SG * IT * 16 + (SG == 4 ? 1024 : 512) / 8 * RT * 16);
    if (err != hipSuccess) return err;
    attr = true;
  }
  const size_t lds = (size_t)2 * SG * IT * 16 + (size_t)(Dh / 8) * RT * 16;
  const dim3 grid((unsigned)((a.n + RT - 1) / RT), (unsigned)a.splits);
  hipLaunchKernelGGL((ts_scan_kernel<CAP, SG>), grid, dim3(256), lds, s, a,
                     reinterpret_cast<const u32x4*>(image), W, Dh);
  return hipGetLastError();
}

template <int CAP>
hipError_t launch_scan_cap(const RecommendArgs& a, const void* image, int64_t W, int Dh,
                           hipStream_t s) {
  // 64-column slabs where two of them fit beside the query block
  return Dh > 512 ? launch_scan<CAP, 4>(a, image, W, Dh, s) : launch_scan<CAP, 8>(a, image, W, Dh, s);
}

}  // namespace

size_t two_stage_image_bytes(int64_t m, int Dp) {
  return (size_t)((m + IT - 1) / IT) * IT * (size_t)two_stage_dh(Dp) * 2;
}

hipError_t launch_two_stage_convert(const float* T, int64_t m, int Dp, void* image, double* norms,
                                    unsigned long long* stats, hipStream_t s) {
  if (m < 1 || !T || !image || !norms || !stats || Dp < 8 || Dp > 1024 || (Dp & 7))
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ts_convert_kernel, dim3((unsigned)((m + IT - 1) / IT)), dim3(256), 0, s, T, m,
                     Dp, two_stage_dh(Dp), reinterpret_cast<u32x4*>(image), norms, stats);
  return hipGetLastError();
}

hipError_t launch_two_stage_scan(const RecommendArgs& a, const void* image, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.k < 1 || a.k > 1024 || a.m < 1 || a.splits < 1 ||
      a.splits > recommend_max_splits(a.k, a.m) || !a.X || !image || !a.maskw || !a.cand ||
      !a.counts || !a.out_items || a.Dp < 8 || a.Dp > 1024 || (a.Dp & 7) || a.inv || a.skip_self)
    return hipErrorInvalidValue;
  const int64_t W = recommend_words(a.m);
  hipError_t e = hipSuccess;
  if (a.bitmap) {
    if (!a.row_ptr || !a.col) return hipErrorInvalidValue;
    e = launch_history_bits(a.row_ptr, a.col, a.qrows, a.r0, a.n, a.m, a.bitmap, s);
    if (e != hipSuccess) return e;
  }
  const int Dh = two_stage_dh(a.Dp), cap = recommend_cap(a.k);
  switch (cap) {
    case 512: e = launch_scan_cap<512>(a, image, W, Dh, s); break;
    case 1024: e = launch_scan_cap<1024>(a, image, W, Dh, s); break;
    default: e = launch_scan_cap<2048>(a, image, W, Dh, s); break;
  }
  if (e != hipSuccess) return e;
  return launch_recommend_merge(a, cap, s);
}

hipError_t launch_two_stage_select(const TwoStageSelectArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.pool < 1 || a.pool > kMaxPool || a.k < 1 || a.k > a.pool || !a.X || !a.Y ||
      !a.pool_items || !a.pool_scores || !a.stats || !a.out_items || !a.out_scores ||
      !a.certified || a.Dp < 8 || a.Dp > 1024 || (a.Dp & 7))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ts_select_kernel, dim3((unsigned)a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace frecsys_hip
