// ctx.h -- what every host translation unit of libfrecsys_hip.so shares: the
// context behind the C-ABI's opaque frecsys_ctx, the error path, the work
// accounting, the call timer, and the helpers of capi.hip that the solve
// drivers of train.hip use too.  Internal header.  The functions that are
// neither templates nor inline are defined once, in capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/frecsys_hip.h"
#include "device_buf.h"
#include "kernels.h"

namespace frecsys_hip {

struct Timer {
  double total_ms = 0.0;
  int64_t launches = 0;
};

// Algorithmic work the library launched under a timer key (SURVEY 8(d)
// definitions, logical dim d; frecsys_work), accumulated per launch.
struct Work {
  double flops = 0.0, bytes = 0.0;
  int64_t entities = 0, launches = 0;
};

// A per-entity vector the host hands over on every call: its device copy
// and the pinned staging buffer upload() fills it through.
struct UploadBuf {
  DevBuf<float> dev;
  PinnedBuf<float> stage;
};

}  // namespace frecsys_hip

using namespace frecsys_hip;  // every includer is host code of the library

// Members are destroyed last to first: the streams and events are declared
// before every buffer, so they outlive them (frecsys_ctx_destroy
// synchronises the streams, then deletes the context with its device
// current).
struct frecsys_ctx {
  int dim = 0, Dp = 0, device = 0, quirks = 1;
  int64_t n[3] = {0, 0, 0};
  Stream stream;
  // history-space (dual) path: a second stream for the concurrent d-space
  // solve of the long histories, and a second lane of history-space buckets
  Stream stream2, stream3;
  hipStream_t stream5 = nullptr;  // early basis builds: an alias of stream3
  Event ev0, ev1;
  Event ev_fork, ev_join, ev_fork3, ev_join3;
  Event ev_pre5, ev_eager[2];
  std::vector<Event> events;  // owner of every pooled event (pool_event)
  DevBuf<float> emb[3];
  DevBuf<float> snap[2];
  DevBuf<float> gram[2];
  DevBuf<int64_t> rp[3];
  DevBuf<int32_t> col[3];
  int64_t nnz[3] = {0, 0, 0};
  std::vector<int64_t> host_rp[2];
  std::vector<int64_t> bounds[2];
  // per-entity vectors (device)
  UploadBuf d_entity_weight, d_entity_reg, d_other_weight, d_gram_w;
  DevBuf<float> d_partials;   // Gramian leaf workspace
  DevBuf<float> d_gslabs[3];  // Gramian group slabs per side (2: train stats)
  GramPlan gplan[2];             // plan of the last Gramian formed per side
  int gram_own[2][2] = {{0, 0}, {0, 0}};  // ... and the groups this rank computed
  DevBuf<float> d_loss;
  DevBuf<float> d_quad;
  DevBuf<unsigned long long> d_fail;
  DevBuf<unsigned int> d_counter;
  // cumulative event counters (frecsys_counter): [0] tagged-word polls that
  // timed out on the device (common.h tpoll); history-space reruns on host
  DevBuf<unsigned int> d_events;
  int64_t hspace_reruns = 0;
  // FRECSYS_DUAL_PROF diagnostics: cycle counters of the wide / tiled
  // d-space solve and of the history-space buckets
  DevBuf<unsigned long long> w_prof, d_prof, dual_prof;
  // per side: the rank's entities in decreasing-history order (LPT queue)
  DevBuf<QueueRec> d_order[3];
  int64_t order_n[3] = {0, 0, 0};
  bool order_stale[3] = {true, true, true};
  std::vector<int64_t> host_rp_eval;
  ncclComm_t comm = nullptr;
  int world = 1, rank = 0;
  std::string err;
  int64_t err_entity = -1;
  std::map<std::string, Timer> timers;
  std::map<std::string, Work> work;
  // history-space (dual) path: the basis of each side's Gramian, the rotated
  // copy of each side, and the solved rows in the rotated basis
  DevBuf<float> q[2];      // Dp x Dp
  DevBuf<float> tri[2];    // [2 * Dp]: diagonal, subdiagonal
  DevBuf<float> refl[2];   // Dp x Dp reflectors + [Dp] tau
  DevBuf<float> xrot[2];   // n_s x Dp
  DevBuf<char> qsplit[2][2];  // split images of Q, Q^T
  DevBuf<char> gsplit;  // split image of G[ITEM] for the wide user loss
  DevBuf<float> out_rot[3];
  DevBuf<float> dual_table;  // [entities][3][Dp] LDL^T factors
  // wide dims (Dp = 512 / 1024): tridiagonalisation work, d-space workspace
  DevBuf<float> tri_work;
  DevBuf<int32_t> d_rix[2];  // iALS++: rating index per CSR entry
  DevBuf<float> d_pred[2];   // iALS++: training / EVAL prediction vectors
  DevBuf<float> d_resid;
  // sharded iALS++ / SAFER2++ block steps: the block columns of the side's
  // rows before the step ([n][bw]), for the prediction refresh of the rows
  // other ranks solve (frecsys_pp_step with RCCL; frecsys_pp_sync without)
  DevBuf<float> d_pp_old;
  int pp_old_side = -1, pp_old_start = 0, pp_old_bw = 0;
  // external-exchange transport (frecsys_set_transport): the in-call
  // exchanges of a sharded call without a communicator
  frecsys_transport transport{};
  bool has_transport = false;
  std::vector<int32_t> pp_order_all[2];  // every row of the side by decreasing h (stable)
  DevBuf<float> d_resid_e;       // per-entity residuals [n] of a sharded pp_step
  DevBuf<float> d_rows;          // train stats: per-row values
  DevBuf<float> d_gstat;         // train stats: U^T U, V^T V
  DevBuf<double> d_dot;
  DevBuf<float> d_scores;        // evaluation: [batch][items] scores
  DevBuf<int32_t> d_topk;        // [eval rows][k]
  DevBuf<char> d_rec;            // the ranking calls' workspace (serve.hip carves it per call)
  DevBuf<float> d_sim_inv;       // frecsys_similar: inverse row norms of the side searched
  DevBuf<int32_t> d_samp_ids;    // frecsys_sampled_metrics: the candidate ids of a row batch
  // frecsys_recommend_two_stage: the item table's bf16 image, its row norms
  // and {largest norm bits, subnormal count}, rebuilt by every call; the rows
  // certified and the rows re-run exactly so far (frecsys_counter)
  DevBuf<char> d_ts_img;
  DevBuf<double> d_ts_norm;
  DevBuf<unsigned long long> d_ts_stats;
  int64_t ts_certified = 0, ts_fallback_rows = 0;
  int64_t rec_splits = 0;       // item splits of the last call (frecsys_counter "recommend_splits")
  // conjugate-gradient path (frecsys_solve_side_cg): i of the last CG call
  // per row of each side (device scratch + host copy; -1: not solved here),
  // the kernel's {sum of i, entities at the cap} and the cumulative counters
  DevBuf<int32_t> d_cg_iters;
  DevBuf<unsigned long long> d_cg_stats;
  DevBuf<int32_t> d_cg_bstart;  // batches of the queue (cg_plan_batches)
  std::vector<int32_t> cg_bstart;
  std::vector<int32_t> cg_iters[3];
  int64_t cg_iterations = 0, cg_unconverged = 0;
  DevBuf<float> wide_ws;         // [wide batch][wide_slot_floats(Dp)]
  // the pre-split copy of the other side for the wide d-space SYRK
  // (wide_syrk.hip; FRECSYS_WIDE_PRESPLIT=0: the register-staged SYRK)
  DevBuf<char> wide_xs;
  // the history-space wide bucket (dual.hip, 256 < h_eff <= 512): split Z
  // fragments, Cholesky slots of S, z
  DevBuf<char> dw_zs;
  DevBuf<float> dw_slots;
  DevBuf<float> dw_z;
  bool wide_presplit = true;
  // FRECSYS_WIDE_WS_MB: the budget of EACH of the wide workspaces (the batch
  // workspace of A tiles, the long-history slabs, the history-space wide
  // bucket), each allocated only as large as its batch needs (8 GB instead of
  // 4 measured 0.6 % faster at MSD and config 5, 16 GB another 1.5 % at
  // config 5 -- fewer, fuller batches).  Each is also capped at a quarter of
  // the device memory free when it is sized (ws_budget), and a failed
  // allocation halves its batch instead of failing the call (ensure_batch);
  // the pre-split table of the other side ((n_other + 1) (6 Dp + 128) B:
  // 12.6 GB for config 5's 2M users) falls back to the register-staged SYRK
  // (bit-identical) when it does not fit.  At the default, the three
  // workspaces and the table take <= 61 GB of 288 at config 5.
  int64_t wide_ws_mb = 16384;
  bool ws_free_cap = true;   // FRECSYS_WS_FREE_CAP=0: no free-memory cap (tests of the OOM path)
  int64_t ws_shrinks = 0;    // allocations cut by a failed hipMalloc (frecsys_counter "ws_shrinks")
  // long-history split of the d-space solve
  int split_rows = 4096;         // rows per partial SYRK (FRECSYS_SPLIT_ROWS, 0 = off; swept 512..4096 at ML-20M d=256: 4096 best)
  std::vector<int2> h_split;
  std::vector<SplitWork> h_work;
  DevBuf<int2> d_split;
  DevBuf<SplitWork> d_work;
  DevBuf<float> d_slabs;
  std::vector<int32_t> order_h[3];      // history lengths in queue order
  std::vector<QueueRec> h_order[3];      // host copy of each side's queue (source of its upload)
  int dual_on = 1;
  // Content versions (every write of a side's embeddings or Gramian takes a
  // fresh number): a Gramian recomputed from unchanged embeddings is reused
  // (the computation is deterministic, the result would be identical), and
  // a basis / rotated copy is rebuilt only when its inputs changed.  When a
  // Gramian is formed for a side whose consumer last took the history-space
  // path, its basis is built right away on stream5 (e.g. during the user
  // loss and the host's xi / omega math between epochs) instead of on the
  // next solve's critical path.
  uint64_t ver_counter = 0;
  uint64_t emb_ver[3] = {0, 0, 0};
  uint64_t gram_ver[2] = {0, 0};
  uint64_t gram_src[2] = {0, 0};    // emb_ver the Gramian was formed from (0: not reusable)
  uint64_t basis_gram[2] = {0, 0};  // gram_ver the basis (T, Q, Q pieces) belongs to
  uint64_t xrot_emb[2] = {0, 0};    // emb_ver of the rotated copy (0: stale / snapshot)
  uint64_t xrot_gram[2] = {0, 0};   // ... and the basis it was rotated into
  uint64_t xrot_sub[2] = {0, 0};    // ... and the row subset it covers (0: every row)
  // Row subsets of the forward rotation: the rows of the other side that a
  // consumer side's history-space entities read (its shard's queue positions
  // [key0, key1)).  At N ranks a shard's short histories touch a fraction of
  // the other side, so the replicated rotation shrinks with N.  Built once
  // per (queue, split point) -- the histories do not change between epochs.
  DevBuf<QueueRec> d_hrows[3];
  int64_t n_hrows[3] = {-1, -1, -1};  // rows in the subset; -1: none (every row)
  int64_t hrows_key[3][2] = {{-1, -1}, {-1, -1}, {-1, -1}};
  // Prefix sums over each side's queue of h_eff, h_eff^2, h_eff^3 and the
  // non-empty count (two variants: with / without the ProjectV tail rows):
  // the frecsys_work accounting of any queue range in O(1) instead of a host
  // loop over the entities on every solve.  Rebuilt with the queue.
  struct WorkPrefix {
    bool valid = false;
    std::vector<double> h1, h2, h3;
    std::vector<int64_t> nz;
  };
  WorkPrefix wprefix[3][2];
  uint64_t hrows_gen[3] = {0, 0, 0};  // subset id (0: every row)
  DevBuf<uint8_t> d_mark;
  bool dual_used[3] = {false, false, false};  // the side's last solve took history space
  int eager_on = 1;                 // FRECSYS_EAGER=0: no early basis builds (A/B)
  // Basis kind per side: 0 = tridiagonal (G = Q T Q^T, any mu / lambda per
  // entity), 1 = Cholesky of the one M = mu*G + lam*I every entity of the
  // consumer's launch shares (q[] then holds L^-T, tri[][0] its status).
  // want_*: what the consumer's last history-space solve used (early builds).
  int basis_mode[2] = {0, 0};
  float basis_mu[2] = {0.f, 0.f}, basis_lam[2] = {0.f, 0.f};
  int want_mode[2] = {0, 0};
  float want_mu[2] = {0.f, 0.f}, want_lam[2] = {0.f, 0.f};
  int chol_basis_on = 1;            // FRECSYS_CHOL_BASIS=0: always tridiagonal (A/B, tests)
  DevBuf<float> chol_work;
  bool eager_pending[2] = {false, false};
  int dual_max_h = 256;  // longest h_eff on the history-space path (set per Dp at create)
  int dual_max_h_side[3] = {256, 256, 256};  // per solved side (FRECSYS_DUAL_MAX_H_USER / _ITEM)
  int dual_serial = 0;  // FRECSYS_DUAL_SERIAL=1: no stream overlap (profiling)
  int debug_skip = 0;   // FRECSYS_DEBUG_SKIP ablation mask (-DFRECSYS_ABLATION builds only)
  int chol_sched = 1;   // FRECSYS_CHOL_SCHED=0: the round-robin worker order (profiling)
  // per-kernel event pairs, resolved after the call's final synchronisation
  struct Pending {
    std::string name;
    hipEvent_t a, b;
  };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> event_pool;  // idle handles of `events`
};

namespace frecsys_hip {

// Records the message as the context's and the process's last error
// (frecsys_last_error) and returns the code.
int fail(frecsys_ctx* c, int code, const std::string& msg);

#define HIP_TRY(c, expr)                                                            \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess)                                                           \
      return fail((c), FRECSYS_ERR_HIP,                                             \
                  std::string(#expr) + ": " + hipGetErrorString(_e));               \
  } while (0)

#define NCCL_TRY(c, expr)                                                           \
  do {                                                                              \
    ncclResult_t _r = (expr);                                                       \
    if (_r != ncclSuccess)                                                          \
      return fail((c), FRECSYS_ERR_RCCL,                                            \
                  std::string(#expr) + ": " + ncclGetErrorString(_r));              \
  } while (0)

void add_work(frecsys_ctx* c, const std::string& key, double flops, double bytes,
              int64_t entities);

// Contiguous nnz-balanced split: rank r gets rows whose prefix nnz falls in
// [r*nnz/P, (r+1)*nnz/P).
void partition_rows(int64_t n_rows, const int64_t* row_ptr, int parts, int64_t* bounds);

// DevBuf::reserve as a call's status.  A buffer that still holds memory
// after a failure is one whose hipFree failed.
template <typename T>
int ensure(frecsys_ctx* c, DevBuf<T>& b, size_t count) {
  const hipError_t e = b.reserve(count);
  if (e == hipSuccess) return FRECSYS_OK;
  return fail(c, FRECSYS_ERR_HIP,
              std::string(b ? "hipFree(*p): "
                            : "hipMalloc((void**)p, sizeof(T) * std::max<size_t>(count, 1)): ") +
                  hipGetErrorString(e));
}

// From here on: what capi.hip shares with train.hip alone.  Hidden, so the
// library's dynamic symbols stay the C-ABI and what they were.
#pragma GCC visibility push(hidden)

// ensure() that reports an out-of-memory hipMalloc instead of failing
// (DevBuf::try_reserve): *oom is set and the buffer left empty.
template <typename T>
int try_ensure(frecsys_ctx* c, DevBuf<T>& b, size_t count, bool* oom) {
  const hipError_t e = b.try_reserve(count, oom);
  if (e == hipSuccess) return FRECSYS_OK;
  return fail(c, FRECSYS_ERR_HIP,
              std::string(b ? "hipFree(*p): " : "hipMalloc: ") + hipGetErrorString(e));
}

// A fresh allocation of `count` elements whatever the buffer held (a table
// replaced as a whole: CSR arrays, queues).
template <typename T>
hipError_t renew(DevBuf<T>& b, size_t count) {
  const hipError_t e = b.release();
  return e != hipSuccess ? e : b.reserve(count);
}

// The wide workspaces' budget and the room a cut one leaves (capi.hip).
size_t ws_budget(frecsys_ctx* c, size_t held);
bool below_headroom();

// A workspace of *batch slots of `per` elements: a failed hipMalloc halves
// the batch (counted in ws_shrinks) until one slot does not fit either, and a
// batch that fits only after such a cut is halved on while it leaves less
// than kRuntimeHeadroom free.  Entities are independent, so the batch size
// never changes a result.
template <typename T>
int ensure_batch(frecsys_ctx* c, DevBuf<T>& b, size_t per, int64_t* batch) {
  bool cut = false;
  while (true) {
    bool oom = false;
    int rc = try_ensure(c, b, per * (size_t)*batch, &oom);
    if (rc) return rc;
    if (!oom) {
      if (!cut || *batch <= 1 || !below_headroom()) return FRECSYS_OK;
      HIP_TRY(c, b.release());
    } else if (*batch <= 1) {
      return fail(c, FRECSYS_ERR_HIP, "hipMalloc: out of memory for one workspace slot");
    }
    *batch = (*batch + 1) / 2;
    ++c->ws_shrinks;
    cut = true;
  }
}

// h_eff: the rows of the other side that the assembly of an entity with h
// history entries reads (vq: the V kinds, whose tail quirk rounds a history
// above 128 up to whole 128-row blocks).  Monotone in h.
inline int64_t queue_heff(int quirks, bool vq, int64_t h) {
  return (vq && quirks && h > 128 && (h % 128) != 0) ? h + 128 - (h % 128) : h;
}
struct HeffSums {
  double h1 = 0, h2 = 0, h3 = 0;
  int64_t nz = 0;
};

// Shared by capi.hip and train.hip; each is described at its definition.
bool valid_side(int side);
void shard(const frecsys_ctx* c, int side, int64_t* lo, int64_t* hi);
int build_order(frecsys_ctx* c, int side);
HeffSums heff_sums(frecsys_ctx* c, int side, bool vq, int64_t lo, int64_t hi);
int join_eager(frecsys_ctx* c, int mask, hipStream_t s);
void emb_written(frecsys_ctx* c, int side);
int prepare_basis(frecsys_ctx* c, int other, const float* X, hipStream_t s, int mode = 0,
                  float mu = 0.f, float lam = 0.f, const QueueRec* rows = nullptr,
                  int64_t nrows = 0, uint64_t sub = 0);
int hspace_rows(frecsys_ctx* c, int side, int other, int64_t q0, int64_t q1,
                const QueueRec** rows, int64_t* nrows, uint64_t* sub);
int allgather_rows(frecsys_ctx* c, float* base, int side, int64_t ld);
bool in_call_exchange(const frecsys_ctx* c);
int xchg_rows(frecsys_ctx* c, float* base, int side, int64_t ld);
int xchg_min_u64(frecsys_ctx* c, unsigned long long* dval);
int upload(frecsys_ctx* c, UploadBuf& b, const float* host, size_t n);
size_t ktimer_begin(frecsys_ctx* c, const std::string& name, hipStream_t s);
void ktimer_end(frecsys_ctx* c, size_t i, hipStream_t s);
void flush_ktimers(frecsys_ctx* c);

#pragma GCC visibility pop

struct ScopedTimer {
  frecsys_ctx* c;
  const char* name;
  ScopedTimer(frecsys_ctx* c_, const char* n_) : c(c_), name(n_) {
    (void)hipEventRecord(c->ev0, c->stream);
  }
  // The end of the timed work, for a caller that has host work to do while
  // the device runs: mark(), the host work, then finish().
  void mark() { (void)hipEventRecord(c->ev1, c->stream); }
  // Stops the timer: synchronises on the end event and accumulates.
  void stop() {
    mark();
    finish();
  }
  void finish() {
    (void)hipEventSynchronize(c->ev1);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) {
      Timer& t = c->timers[name];
      t.total_ms += ms;
      t.launches += 1;
    }
  }
};

}  // namespace frecsys_hip
