// cg.hip -- per-entity conjugate-gradient solve on gfx950 (--use_cg).
//
// Replaces the `Eigen::ConjugateGradient<MatrixXf, Lower>` branch of the
// reference's Project / ProjectU / ProjectV (ials.h:133-139,
// safer2.h:152-157, 210-215): Jacobi-preconditioned CG from a zero start on
//   A = s_G G + sum_j c_j y_j y_j^T + lambda I,   b = sum_j bw_j y_j
// that never forms A.  Per kind (the assembly of solve.hip, common.h):
//   iALS        s_G = w        c_j = 1         bw_j = 1
//   WEIGHTED_U  s_G = omega w  c_j = omega/h   bw_j = omega/h
//   WEIGHTED_V  s_G = w        c_j = nu_j      bw_j = nu_j  (tail-quirk rows:
//               in c_j a second time, not in b -- solve.hip's virtual rows)
// Recurrence (Eigen's conjugate_gradient, ConjugateGradient.h):
//   x = 0; r = b; ||b||^2 == 0 -> x = 0, 0 iterations
//   thr = max(tol^2 ||b||^2, FLT_MIN); ||r||^2 < thr -> done
//   p = r ./ diag(A); rho = r.p; i = 0
//   while i < max_iterations:
//     t = A p; alpha = rho / (p.t); x += alpha p; r -= alpha t
//     if ||r||^2 < thr: break
//     z = r ./ diag(A); rho' = r.z; p = z + (rho'/rho) p; rho = rho'; ++i
// (a zero diagonal entry has inverse 1).
//
// One workgroup (4 waves) takes a batch of up to kCgE = 16 consecutive
// entities of the LPT queue (cg_plan_batches: fewer where the histories are
// long, so the longest entities do not queue behind each other on one CU; the
// histories of a batch are similar in length).  Per iteration:
//   1. T = P G for the whole batch on v_mfma_f32_16x16x4_f32 (exact fp32):
//      the entities are the 16 rows of the A operand (P in LDS), G streams
//      from L2 once per batch; every output element is one accumulator chain
//      over k = 0 .. Dp-1, so an entity's row does not depend on its slot or
//      on the other rows of the batch;
//   2. the history rows: GP lanes per row, 64/GP rows per pass, kCgU passes
//      (one chunk) in flight per wave, the row ids one chunk ahead (measured:
//      cap-3 epoch 51 -> 34 ms); s_j = y_j.p by a butterfly over the
//      row's lanes, t += c_j s_j y_j per lane, the row sub-sums folded by a
//      butterfly.  An entity of at most kCgCoopRows rows is streamed by the
//      wave that owns its slot (slot % 4); a longer one by all four waves,
//      wave w taking the chunks w, w + 4, ..., the four partial sums added in
//      wave order by the owner;
//   3. the owner wave's vector updates and dots of the recurrence (fixed
//      butterflies).
// Every reduction of an entity has an order fixed by (Dp, h) alone: result
// bits do not depend on batch, slot, grid or world size.  r, p, t and the
// inverse diagonal of the batch live in LDS (74 KB at Dp = 256: two
// workgroups per CU), x in the output rows.  A stopped entity is masked out;
// the batch ends when all have stopped.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "common.h"
#include "kernels.h"

namespace frecsys_hip {

namespace {

constexpr int kCgWaves = 4;
constexpr int kCgThreads = 64 * kCgWaves;

typedef float f32x4a __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;
}
// sum over the lanes l ^ o, o = lo, 2 lo, .. < hi (every lane gets the sum)
__device__ __forceinline__ float bfly(float v, int lo, int hi) {
  for (int o = lo; o < hi; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float4 bfly4(float4 v, int lo, int hi) {
  for (int o = lo; o < hi; o <<= 1) {
    v.x += __shfl_xor(v.x, o, 64);
    v.y += __shfl_xor(v.y, o, 64);
    v.z += __shfl_xor(v.z, o, 64);
    v.w += __shfl_xor(v.w, o, 64);
  }
  return v;
}

struct CgEntity {
  int64_t e, h, p0, ntot;
  float lam, sG, cu;
};

__device__ __forceinline__ CgEntity cg_entity(const CgArgs& a, const QueueRec& rec) {
  CgEntity q;
  q.e = rec.entity;
  q.h = rec.h;
  q.p0 = rec.p0;
  int64_t extra = 0;
  if (a.kind == KIND_WEIGHTED_V && a.quirk && q.h > 128 && (q.h % 128) != 0)
    extra = 128 - (q.h % 128);
  q.ntot = q.h + extra;
  const float omega =
      (a.kind == KIND_WEIGHTED_U && a.entity_weight) ? a.entity_weight[q.e] : 1.0f;
  q.lam = entity_lambda(a.kind, a.reg, a.reg_exp, a.w, a.alpha, q.h, a.n_other, a.entity_reg, q.e,
                        a.lambda_is_reg);
  q.sG = a.kind == KIND_WEIGHTED_U ? omega * a.w : a.w;
  q.cu = a.kind == KIND_WEIGHTED_U ? omega / (float)q.h : 1.0f;
  return q;
}

// The chunks c0, c0 + cs, ... of the (virtual) history rows of an entity by
// one wave (a chunk: kCgU passes of 64 / GP rows).
// MODE 0: o0 = sum bw_j y_j (the rhs), o1 = sum c_j y_j.^2 (diagonal part).
// MODE 1: o0 = sum c_j (y_j . p) y_j.
// Lane (sub, cg): rows j = sub (mod RP), columns 4 cg .. 4 cg + 3; on return
// every lane of a column group holds the sums over the wave's rows.
template <int MODE>
__device__ __forceinline__ void cg_stream(const CgArgs& a, const CgEntity& q, int GP, int G4,
                                          int sub, int cg, float4 p4, int c0, int cs, float4& o0,
                                          float4& o1) {
  const int RP = 64 / GP;
  const int Dp = a.Dp;
  const bool vk = a.kind == KIND_WEIGHTED_V;
  const int64_t chunk = (int64_t)RP * kCgU;
  const int64_t step = cs * chunk;
  o0 = f4zero();
  o1 = f4zero();
  // The row ids run one chunk ahead of the rows, so a chunk's row loads do
  // not wait for the id -> row dependency.  Rows past the history load
  // nothing and carry zero coefficients.
  auto load_ids = [&](int64_t j0, int (&id)[kCgU]) {
#pragma unroll
    for (int u = 0; u < kCgU; ++u) {
      const int64_t j = j0 + (int64_t)u * RP + sub;
      id[u] = j < q.ntot ? a.col[q.p0 + (j < q.h ? j : (q.h - 128 + (j - q.h)))] : -1;
    }
  };
  int id[kCgU], idn[kCgU];
  load_ids(c0 * chunk, id);
  for (int64_t j0 = c0 * chunk; j0 < q.ntot; j0 += step) {
    float4 y[kCgU];
    float c[kCgU], bw[kCgU];
#pragma unroll
    for (int u = 0; u < kCgU; ++u) {
      const int64_t j = j0 + (int64_t)u * RP + sub;
      const bool live = id[u] >= 0;
      if (vk) {
        const float nu = a.other_weight[live ? id[u] : 0];
        c[u] = live ? nu : 0.0f;
        bw[u] = (live && j < q.h) ? nu : 0.0f;
      } else {
        c[u] = live ? q.cu : 0.0f;
        bw[u] = c[u];
      }
      y[u] = f4zero();
      if (live && cg < G4)
        y[u] = *reinterpret_cast<const float4*>(a.X + (int64_t)id[u] * Dp + 4 * cg);
    }
    load_ids(j0 + step, idn);
#pragma unroll
    for (int u = 0; u < kCgU; ++u) {
      if (MODE == 0) {
        o0.x += bw[u] * y[u].x, o0.y += bw[u] * y[u].y;
        o0.z += bw[u] * y[u].z, o0.w += bw[u] * y[u].w;
        o1.x += c[u] * (y[u].x * y[u].x), o1.y += c[u] * (y[u].y * y[u].y);
        o1.z += c[u] * (y[u].z * y[u].z), o1.w += c[u] * (y[u].w * y[u].w);
      } else {
        const float s = c[u] * bfly(dot4(y[u], p4), 1, GP);
        o0.x += s * y[u].x, o0.y += s * y[u].y, o0.z += s * y[u].z, o0.w += s * y[u].w;
      }
    }
#pragma unroll
    for (int u = 0; u < kCgU; ++u) id[u] = idn[u];
  }
  o0 = bfly4(o0, GP, 64);
  if (MODE == 0) o1 = bfly4(o1, GP, 64);
}

__global__ void __launch_bounds__(kCgThreads) cg_kernel(CgArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Dp = a.Dp;
  const int LDP = Dp + 4;  // P rows: the 16 x 4 MFMA operand read hits 64 distinct banks
  float* rs = smem;
  float* ts = rs + kCgE * Dp;
  float* ds = ts + kCgE * Dp;
  float* ps = ds + kCgE * Dp;
  float* part = ps + kCgE * LDP;  // [2][kCgWaves][Dp] partial sums of a cooperative stream
  float* s_rho = part + 2 * kCgWaves * Dp;
  float* s_thr = s_rho + kCgE;
  int* s_it = reinterpret_cast<int*>(s_thr + kCgE);
  int* s_act = s_it + kCgE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G4 = Dp / 4;
  int GP = 2;
  while (GP < G4) GP <<= 1;
  const int sub = lane / GP, cg = lane % GP;
  const bool own = sub == 0 && cg < G4;  // this lane holds columns 4 cg .. + 3 of the vectors
  const int64_t pos0 = a.bstart[blockIdx.x];
  const int nE = (int)(a.bstart[blockIdx.x + 1] - pos0);  // 1 .. kCgE entities
  const float4 colmask = make_float4(4 * cg + 0 < a.dim ? 1.f : 0.f, 4 * cg + 1 < a.dim ? 1.f : 0.f,
                                     4 * cg + 2 < a.dim ? 1.f : 0.f, 4 * cg + 3 < a.dim ? 1.f : 0.f);

  auto finish = [&](const CgEntity& q, int slot, int it, bool capped, bool finite) {
    if (lane == 0) {
      s_act[slot] = 0;
      a.iters[q.e] = it;
      if (it) atomicAdd(a.stats, (unsigned long long)it);
      if (capped) atomicAdd(a.stats + 1, 1ull);
      if (!finite) atomicMin(a.fail, (unsigned long long)(q.e + 1));
    }
  };
  // the four waves' partial sums of a cooperative stream, added in wave order
  auto part_put = [&](int k, float4 v) {
    if (own) *reinterpret_cast<float4*>(part + (k * kCgWaves + wave) * Dp + 4 * cg) = v;
  };
  auto part_sum = [&](int k) {
    float4 v = f4zero();
    if (cg < G4) {
      v = *reinterpret_cast<const float4*>(part + (k * kCgWaves + 0) * Dp + 4 * cg);
#pragma unroll
      for (int w = 1; w < kCgWaves; ++w)
        v = f4add(v, *reinterpret_cast<const float4*>(part + (k * kCgWaves + w) * Dp + 4 * cg));
    }
    return v;
  };

  // ---- setup: b, diag(A), the first search direction ----
  // (every branch on slot state below is workgroup-uniform: the barriers of
  // the cooperative streams are reached by all four waves)
  unsigned coopmask = 0;
  for (int slot = 0; slot < kCgE; ++slot) {
    const bool mine = wave == (slot & (kCgWaves - 1));
    if (mine) {
      if (lane == 0) s_act[slot] = 0;
      if (own) *reinterpret_cast<float4*>(ps + slot * LDP + 4 * cg) = f4zero();
    }
    if (slot >= nE) continue;
    const QueueRec rec = a.order[pos0 + slot];
    if (rec.h == 0) continue;  // empty history: row untouched, iterations stay -1
    const CgEntity q = cg_entity(a, rec);
    const bool coop = q.ntot > kCgCoopRows;
    float4 b4 = f4zero(), d4 = f4zero();
    if (coop) {
      coopmask |= 1u << slot;
      cg_stream<0>(a, q, GP, G4, sub, cg, f4zero(), wave, kCgWaves, b4, d4);
      part_put(0, b4);
      part_put(1, d4);
      __syncthreads();
      if (mine) {
        b4 = part_sum(0);
        d4 = part_sum(1);
      }
      __syncthreads();
    } else if (mine) {
      cg_stream<0>(a, q, GP, G4, sub, cg, f4zero(), 0, 1, b4, d4);
    }
    if (!mine) continue;
    float4 g4 = f4zero();
    if (own) {
      g4.x = a.G[(int64_t)(4 * cg + 0) * Dp + 4 * cg + 0];
      g4.y = a.G[(int64_t)(4 * cg + 1) * Dp + 4 * cg + 1];
      g4.z = a.G[(int64_t)(4 * cg + 2) * Dp + 4 * cg + 2];
      g4.w = a.G[(int64_t)(4 * cg + 3) * Dp + 4 * cg + 3];
    }
    float4 inv;
    {
      const float dx = (q.sG * g4.x + d4.x) + q.lam, dy = (q.sG * g4.y + d4.y) + q.lam;
      const float dz = (q.sG * g4.z + d4.z) + q.lam, dw = (q.sG * g4.w + d4.w) + q.lam;
      inv = make_float4(dx != 0.f ? 1.0f / dx : 1.0f, dy != 0.f ? 1.0f / dy : 1.0f,
                        dz != 0.f ? 1.0f / dz : 1.0f, dw != 0.f ? 1.0f / dw : 1.0f);
    }
    if (!own) b4 = f4zero();
    const float bn2 = bfly(dot4(b4, b4), 1, 64);
    const float thr = fmaxf(a.tol * a.tol * bn2, FLT_MIN);
    if (bn2 == 0.0f || bn2 < thr || a.max_iter == 0) {
      if (own) *reinterpret_cast<float4*>(a.out + q.e * Dp + 4 * cg) = f4zero();
      finish(q, slot, 0, !(bn2 == 0.0f || bn2 < thr), true);
      continue;
    }
    const float4 p4 = make_float4(b4.x * inv.x, b4.y * inv.y, b4.z * inv.z, b4.w * inv.w);
    const float rho = bfly(dot4(b4, p4), 1, 64);
    if (own) {
      *reinterpret_cast<float4*>(rs + slot * Dp + 4 * cg) = b4;
      *reinterpret_cast<float4*>(ds + slot * Dp + 4 * cg) = inv;
      *reinterpret_cast<float4*>(ps + slot * LDP + 4 * cg) = p4;
    }
    if (lane == 0) {
      s_rho[slot] = rho;
      s_thr[slot] = thr;
      s_it[slot] = 0;
      s_act[slot] = 1;
    }
  }
  __syncthreads();

  const int nct = (Dp + 15) / 16;  // 16-column tiles of T
  const int mi = lane & 15, mk = lane >> 4;
  while (true) {
    // the active slots of this iteration, read before anyone changes them
    // (the flags change only after the next barrier): the same in every thread
    unsigned act = 0;
#pragma unroll
    for (int s = 0; s < kCgE; ++s) act |= (s_act[s] ? 1u : 0u) << s;
    if (!act) break;

    // ---- T = P G: wave w owns the column tiles w, w + 4, w + 8, w + 12 ----
    {
      f32x4a acc[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = f32x4a{0.f, 0.f, 0.f, 0.f};
      const float* prow = ps + mi * LDP + mk;
      for (int k0 = 0; k0 < Dp; k0 += 4) {
        const float av = prow[k0];
        const float* grow = a.G + (int64_t)(k0 + mk) * Dp + mi;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int n0 = 16 * (wave + kCgWaves * m);
          if (n0 < Dp) {  // wave-uniform
            const float bv = (n0 + mi < Dp) ? grow[n0] : 0.0f;
            acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[m], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int ct = wave + kCgWaves * m;
        if (ct < nct && 16 * ct + mi < Dp) {
#pragma unroll
          for (int v = 0; v < 4; ++v) ts[(4 * mk + v) * Dp + 16 * ct + mi] = acc[m][v];
        }
      }
    }
    __syncthreads();

    // ---- per entity: history stream, then the recurrence ----
    for (int slot = 0; slot < nE; ++slot) {
      if (!(act >> slot & 1)) continue;
      const bool mine = wave == (slot & (kCgWaves - 1));
      const bool coop = coopmask >> slot & 1;
      if (!coop && !mine) continue;
      const CgEntity q = cg_entity(a, a.order[pos0 + slot]);
      float4 p4 = f4zero();
      if (cg < G4) p4 = *reinterpret_cast<const float4*>(ps + slot * LDP + 4 * cg);
      float4 th, unused;
      if (coop) {
        cg_stream<1>(a, q, GP, G4, sub, cg, p4, wave, kCgWaves, th, unused);
        part_put(0, th);
        __syncthreads();
        if (mine) th = part_sum(0);
        __syncthreads();
        if (!mine) continue;
      } else {
        cg_stream<1>(a, q, GP, G4, sub, cg, p4, 0, 1, th, unused);
      }
      const int it = s_it[slot];
      const float rho = s_rho[slot], thr = s_thr[slot];
      float4 t4 = f4zero(), r4 = f4zero(), inv = f4zero();
      if (own) {
        const float4 g = *reinterpret_cast<const float4*>(ts + slot * Dp + 4 * cg);
        r4 = *reinterpret_cast<const float4*>(rs + slot * Dp + 4 * cg);
        inv = *reinterpret_cast<const float4*>(ds + slot * Dp + 4 * cg);
        t4.x = colmask.x * ((q.sG * g.x + th.x) + q.lam * p4.x);
        t4.y = colmask.y * ((q.sG * g.y + th.y) + q.lam * p4.y);
        t4.z = colmask.z * ((q.sG * g.z + th.z) + q.lam * p4.z);
        t4.w = colmask.w * ((q.sG * g.w + th.w) + q.lam * p4.w);
      } else {
        p4 = f4zero();
      }
      const float alpha = rho / bfly(dot4(p4, t4), 1, 64);
      float4 x4 = f4zero();
      if (own) {
        float* xo = a.out + q.e * Dp + 4 * cg;
        if (it > 0) x4 = *reinterpret_cast<const float4*>(xo);
        x4.x += alpha * p4.x, x4.y += alpha * p4.y, x4.z += alpha * p4.z, x4.w += alpha * p4.w;
        *reinterpret_cast<float4*>(xo) = x4;
        r4.x -= alpha * t4.x, r4.y -= alpha * t4.y, r4.z -= alpha * t4.z, r4.w -= alpha * t4.w;
      }
      const float rn2 = bfly(dot4(r4, r4), 1, 64);
      const bool conv = rn2 < thr;
      const bool capped = !conv && it + 1 >= a.max_iter;
      if (conv || capped) {
        // x - x is 0 for finite x, NaN otherwise
        const float bad = bfly(fabsf(x4.x - x4.x) + fabsf(x4.y - x4.y) + fabsf(x4.z - x4.z) +
                                   fabsf(x4.w - x4.w), 1, 64);
        finish(q, slot, conv ? it : it + 1, capped, bad == 0.0f);
        continue;
      }
      const float4 z4 = make_float4(r4.x * inv.x, r4.y * inv.y, r4.z * inv.z, r4.w * inv.w);
      const float rho1 = bfly(dot4(r4, z4), 1, 64);
      const float beta = rho1 / rho;
      if (own) {
        p4.x = z4.x + beta * p4.x, p4.y = z4.y + beta * p4.y;
        p4.z = z4.z + beta * p4.z, p4.w = z4.w + beta * p4.w;
        *reinterpret_cast<float4*>(rs + slot * Dp + 4 * cg) = r4;
        *reinterpret_cast<float4*>(ps + slot * LDP + 4 * cg) = p4;
      }
      if (lane == 0) {
        s_rho[slot] = rho1;
        s_it[slot] = it + 1;
      }
    }
    __syncthreads();
  }
}

}  // namespace

size_t cg_lds_bytes(int Dp) {
  return sizeof(float) * ((size_t)kCgE * (3 * Dp + Dp + 4) + (size_t)2 * kCgWaves * Dp + 2 * kCgE) +
         sizeof(int) * 2 * kCgE;
}

void cg_plan_batches(const QueueRec* order, int64_t n, std::vector<int32_t>* bstart) {
  bstart->clear();
  bstart->push_back(0);
  int64_t i = 0;
  while (i < n) {
    int64_t rows = 0;
    int cnt = 0;
    while (i < n && cnt < kCgE && (cnt == 0 || rows + order[i].h <= kCgBatchRows)) {
      rows += order[i].h;
      ++cnt;
      ++i;
    }
    bstart->push_back((int32_t)i);
  }
}

hipError_t launch_cg(const CgArgs& a, hipStream_t s) {
  if (a.n_batches <= 0) return hipSuccess;
  const size_t lds = cg_lds_bytes(a.Dp);
  static bool attr = false;
  if (!attr) {
    hipError_t err = hipFuncSetAttribute((const void*)cg_kernel,
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)cg_lds_bytes(256));
    if (err != hipSuccess) return err;
    attr = true;
  }
  hipLaunchKernelGGL(cg_kernel, dim3((unsigned)a.n_batches), dim3(kCgThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace frecsys_hip
