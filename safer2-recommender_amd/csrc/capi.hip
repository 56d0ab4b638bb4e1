// capi.hip -- host side of libfrecsys_hip.so: the C-ABI declared in
// include/frecsys_hip.h.  Owns the device state of one process (one GPU):
// embeddings (row-major, padded leading dim), Gramians, CSR of each side,
// workspaces, the RCCL communicator, and the HIP stream everything runs on.
//
// Sharding (one process per GPU): every rank keeps full replicas of U and V
// (they fit HBM at every configured size) and owns a contiguous nnz-balanced
// range of users and of items.  A half-step is
//   partial G over own rows -> ncclAllReduce -> solve own rows ->
//   grouped ncclBroadcast of every rank's rows (an all-gather with uneven
//   counts, in place).
//
// What lives here: the context's life cycle, the data loaders, the Gramian
// and its exchange with the basis it feeds (prepare_basis, early builds), the
// losses and train statistics, frecsys_eval_topk, the timers / work / counters
// queries, and the one definition of the functions ctx.h declares.  The solve
// drivers (d-space, history space, wide, CG) and the iALS++ block step are in
// train.hip; the ranking and evaluation calls (frecsys_recommend and what
// followed it) are in serve.hip.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"
#include "wide.h"

namespace {
std::string g_last_error;
}  // namespace

// The one definition of what ctx.h declares for every host translation unit.
namespace frecsys_hip {

int fail(frecsys_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  g_last_error = msg;
  return code;
}

void add_work(frecsys_ctx* c, const std::string& key, double flops, double bytes,
              int64_t entities) {
  Work& w = c->work[key];
  w.flops += flops;
  w.bytes += bytes;
  w.entities += entities;
  w.launches += 1;
}

void partition_rows(int64_t n_rows, const int64_t* row_ptr, int parts, int64_t* bounds) {
  const int64_t nnz = row_ptr[n_rows] - row_ptr[0];
  bounds[0] = 0;
  for (int r = 1; r < parts; ++r) {
    const int64_t target = row_ptr[0] + (nnz * r) / parts;
    const int64_t* it = std::lower_bound(row_ptr, row_ptr + n_rows + 1, target);
    int64_t b = it - row_ptr;
    if (b < bounds[r - 1]) b = bounds[r - 1];
    if (b > n_rows) b = n_rows;
    bounds[r] = b;
  }
  bounds[parts] = n_rows;
}

// Bytes one wide workspace may take now: FRECSYS_WIDE_WS_MB, capped at a
// quarter of the device memory that is free (plus what the workspace
// already holds), so several contexts or other tenants of the device leave
// each other room.
size_t ws_budget(frecsys_ctx* c, size_t held) {
  size_t b = (size_t)c->wide_ws_mb << 20;
  size_t fr = 0, tot = 0;
  if (c->ws_free_cap) {
    if (hipMemGetInfo(&fr, &tot) == hipSuccess)
      b = std::min(b, (fr + held) / 4);
    else
      (void)hipGetLastError();
  }
  return b;
}

// What a workspace that was cut after a failed hipMalloc leaves free.  The
// halving would otherwise stop at the largest size that still fits, i.e. with
// the device full to within that size's granularity, and the runtime has
// allocations of its own to make after it: a failed hipMalloc makes it give
// back the idle queues' scratch memory, and the next kernel with a private
// segment (wide_syrk2_kernel: 20..28 B per lane, a 2 KiB granule per wave x 32
// waves x 256 CUs x 8 XCCs = 128 MiB for a grid that fills the device) has its
// dispatch aborted with HSA_STATUS_ERROR_OUT_OF_RESOURCES when that scratch
// cannot be allocated again.  512 MiB: four times that, and room for the
// pre-split table of a short other side, which is allocated behind the cut
// workspaces without a cut of its own.
constexpr size_t kRuntimeHeadroom = (size_t)512 << 20;
bool below_headroom() {
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return fr < kRuntimeHeadroom;
}

bool valid_side(int side) { return side >= 0 && side <= 2; }

static void refresh_bounds(frecsys_ctx* c, int side) {
  if (side > 1) return;
  c->bounds[side].assign(c->world + 1, 0);
  if (!c->host_rp[side].empty()) {
    partition_rows(c->n[side], c->host_rp[side].data(), c->world, c->bounds[side].data());
  } else {
    for (int r = 0; r <= c->world; ++r) c->bounds[side][r] = c->n[side] * r / c->world;
  }
}

void shard(const frecsys_ctx* c, int side, int64_t* lo, int64_t* hi) {
  if (side > 1 || c->world == 1 || c->bounds[side].empty()) {
    *lo = 0;
    *hi = c->n[side];
    return;
  }
  *lo = c->bounds[side][c->rank];
  *hi = c->bounds[side][c->rank + 1];
}

// Entities of the rank's shard of `side`, longest history first (stable),
// uploaded as the work queue of the tiled solve kernel (one 16-B record per
// entity: id, history length, CSR offset).
int build_order(frecsys_ctx* c, int side) {
  if (!c->order_stale[side] && c->d_order[side]) return FRECSYS_OK;
  int64_t lo, hi;
  shard(c, side, &lo, &hi);
  const std::vector<int64_t>& rp = side == 2 ? c->host_rp_eval : c->host_rp[side];
  std::vector<int32_t> ord((size_t)(hi - lo));
  for (int64_t i = lo; i < hi; ++i) ord[i - lo] = (int32_t)i;
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) {
    return (rp[x + 1] - rp[x]) > (rp[y + 1] - rp[y]);
  });
  std::vector<QueueRec>& recs = c->h_order[side];  // lives until the next rebuild (async copy)
  recs.resize(ord.size());
  for (size_t i = 0; i < ord.size(); ++i) {
    const int32_t e = ord[i];
    recs[i].entity = e;
    recs[i].h = (int32_t)(rp[e + 1] - rp[e]);
    recs[i].p0 = rp[e];
  }
  if (renew(c->d_order[side], recs.size()) != hipSuccess)
    return fail(c, FRECSYS_ERR_HIP, "hipMalloc failed (order)");
  if (!recs.empty() && hipMemcpyAsync(c->d_order[side], recs.data(),
                                      sizeof(QueueRec) * recs.size(), hipMemcpyHostToDevice,
                                      c->stream) != hipSuccess)
    return fail(c, FRECSYS_ERR_HIP, "hipMemcpy failed (order)");
  c->order_n[side] = (int64_t)recs.size();
  c->order_h[side].resize(recs.size());
  for (size_t i = 0; i < recs.size(); ++i) c->order_h[side][i] = recs[i].h;
  c->order_stale[side] = false;
  c->wprefix[side][0].valid = c->wprefix[side][1].valid = false;
  c->hrows_key[side][0] = c->hrows_key[side][1] = -1;  // subsets follow the queue
  return FRECSYS_OK;
}

// Sums of h_eff, h_eff^2, h_eff^3 and of the non-empty entities over queue
// positions [lo, hi) of `side` (vq: the V kinds' tail-quirk h_eff).
HeffSums heff_sums(frecsys_ctx* c, int side, bool vq, int64_t lo, int64_t hi) {
  frecsys_ctx::WorkPrefix& p = c->wprefix[side][vq ? 1 : 0];
  const std::vector<int32_t>& hs = c->order_h[side];
  if (!p.valid || p.h1.size() != hs.size() + 1) {
    const size_t n = hs.size();
    p.h1.assign(n + 1, 0.0);
    p.h2.assign(n + 1, 0.0);
    p.h3.assign(n + 1, 0.0);
    p.nz.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
      const double h = (double)queue_heff(c->quirks, vq, hs[i]);
      p.h1[i + 1] = p.h1[i] + h;
      p.h2[i + 1] = p.h2[i] + h * h;
      p.h3[i + 1] = p.h3[i] + h * h * h;
      p.nz[i + 1] = p.nz[i] + (h > 0 ? 1 : 0);
    }
    p.valid = true;
  }
  HeffSums s;
  if (hi <= lo) return s;
  s.h1 = p.h1[hi] - p.h1[lo];
  s.h2 = p.h2[hi] - p.h2[lo];
  s.h3 = p.h3[hi] - p.h3[lo];
  s.nz = p.nz[hi] - p.nz[lo];
  return s;
}

// Stream s waits (on the device) for the early basis builds still running
// on stream5 (mask bit per side).
int join_eager(frecsys_ctx* c, int mask, hipStream_t s) {
  for (int t = 0; t < 2; ++t)
    if ((mask >> t & 1) && c->eager_pending[t]) {
      HIP_TRY(c, hipStreamWaitEvent(s, c->ev_eager[t], 0));
      c->eager_pending[t] = false;
    }
  return FRECSYS_OK;
}
void emb_written(frecsys_ctx* c, int side) { c->emb_ver[side] = ++c->ver_counter; }

// Basis of the other side's Gramian, G = Q T Q^T, and the other side
// rotated into it (X Q): the inputs of the history-space solve.  Rebuilt
// only when the Gramian (basis) or the rows (rotation) changed since.
int prepare_basis(frecsys_ctx* c, int other, const float* X, hipStream_t s, int mode, float mu,
                  float lam, const QueueRec* rows, int64_t nrows, uint64_t sub) {
  const int Dp = c->Dp;
  int rc = ensure(c, c->q[other], (size_t)Dp * Dp);
  if (!rc) rc = ensure(c, c->tri[other], (size_t)2 * Dp);
  if (!rc) rc = ensure(c, c->refl[other], (size_t)Dp * Dp + Dp);
  if (rc) return rc;
  if (mode == 0) mu = lam = 0.f;
  const bool same_kind = c->basis_mode[other] == mode && c->basis_mu[other] == mu &&
                         c->basis_lam[other] == lam;
  const bool need_basis = c->basis_gram[other] == 0 ||
                          c->basis_gram[other] != c->gram_ver[other] || !same_kind;
  const uint64_t xkey = X == c->emb[other] ? c->emb_ver[other] : 0;
  if (!rows) sub = 0;
  const bool need_rot = need_basis || xkey == 0 || c->xrot_emb[other] != xkey ||
                        c->xrot_gram[other] != c->gram_ver[other] ||
                        (c->xrot_sub[other] != 0 && c->xrot_sub[other] != sub);
  const int64_t nrot = rows ? nrows : c->n[other];
  if (s != c->stream5) {
    // an early build of this basis (or one sharing tri_work) may still run
    rc = join_eager(c, 3, s);
    if (rc) return rc;
  }
  if (!need_rot) return FRECSYS_OK;
  rc = ensure(c, c->xrot[other], (size_t)std::max<int64_t>(c->n[other], 1) * Dp);
  if (rc) return rc;
  c->xrot_emb[other] = xkey;
  c->xrot_gram[other] = c->gram_ver[other];
  c->xrot_sub[other] = sub;
  if (!need_basis) {
    HIP_TRY(c, launch_rotate(X, rows, 0, nrot, c->qsplit[other][0], c->xrot[other], Dp,
                             s));
    return FRECSYS_OK;
  }
  c->basis_gram[other] = c->gram_ver[other];
  {  // Cholesky + triangular inverse n^3/3 + n^3/3; Householder reduction 4n^3/3 + Q 4n^3/3
    const double n = Dp;
    add_work(c, mode == 1 ? "basis_chol" : "basis_tridiag",
             mode == 1 ? 2.0 * n * n * n / 3.0 : 8.0 * n * n * n / 3.0, 2.0 * n * n * 4.0, 1);
  }
  c->basis_mode[other] = mode;
  c->basis_mu[other] = mu;
  c->basis_lam[other] = lam;
  for (int t = 0; t < 2; ++t)  // bf16-piece images of the forward and back rotations
    HIP_TRY(c, c->qsplit[other][t].reserve(basis_split_bytes(Dp)));
  if (mode == 1) {
    // q = L^-T: forward X L^-T (image of q), back x' L^-1 (image of q^T)
    rc = ensure(c, c->chol_work, chol_basis_work_floats(Dp));
    if (rc) return rc;
    HIP_TRY(c, launch_chol_basis(c->gram[other], Dp, mu, lam, c->chol_work, c->q[other],
                                 c->tri[other], s));
    HIP_TRY(c, launch_split_basis(c->q[other], Dp, 0, c->qsplit[other][0], s));
    HIP_TRY(c, launch_split_basis(c->q[other], Dp, 1, c->qsplit[other][1], s));
    HIP_TRY(c, launch_rotate(X, rows, 0, nrot, c->qsplit[other][0], c->xrot[other], Dp,
                             s));
    return FRECSYS_OK;
  }
  float* tau = c->refl[other] + (size_t)Dp * Dp;
  const bool qpipe = tridiag_forms_q(Dp);
  if (wide_dim(Dp) || qpipe) {
    rc = ensure(c, c->tri_work, tridiag_work_floats(Dp));
    if (rc) return rc;
  }
  if (qpipe) {
    // Q rows and their split images formed inside the reduction's launch
    HIP_TRY(c, launch_tridiag(c->gram[other], Dp, c->tri[other], c->tri[other] + Dp,
                              c->refl[other], tau, s, c->tri_work, c->q[other],
                              c->qsplit[other][0], c->qsplit[other][1], c->d_events));
    HIP_TRY(c, launch_rotate(X, rows, 0, nrot, c->qsplit[other][0], c->xrot[other], Dp,
                             s));
    return FRECSYS_OK;
  }
  HIP_TRY(c, launch_tridiag(c->gram[other], Dp, c->tri[other], c->tri[other] + Dp, c->refl[other],
                            tau, s, c->tri_work, nullptr, nullptr, nullptr, c->d_events));
  HIP_TRY(c, launch_form_q(c->refl[other], tau, Dp, c->q[other], s, c->qsplit[other][0],
                           c->qsplit[other][1]));
  HIP_TRY(c, launch_rotate(X, rows, 0, nrot, c->qsplit[other][0], c->xrot[other], Dp, s));
  return FRECSYS_OK;
}

// The rows of `other` that side's history-space entities (its queue
// positions [q0, q1)) read: a row list when it is well below the whole
// table, else none (rotate every row).  Marked on the device, compacted on
// the host once per queue and split point (one synchronisation then).
int hspace_rows(frecsys_ctx* c, int side, int other, int64_t q0, int64_t q1,
                const QueueRec** rows, int64_t* nrows, uint64_t* sub) {
  *rows = nullptr;
  *nrows = 0;
  *sub = 0;
  if (q1 <= q0) return FRECSYS_OK;
  if (c->hrows_key[side][0] != q0 || c->hrows_key[side][1] != q1) {
    // an early build may still be rotating with the old list (stream5): the
    // synchronisation below then covers it before the list is rewritten
    int rc = join_eager(c, 3, c->stream);
    if (rc) return rc;
    const int64_t no = c->n[other];
    rc = ensure(c, c->d_mark, (size_t)no);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_mark, 0, (size_t)no, c->stream));
    HIP_TRY(c, launch_mark_rows(c->d_order[side] + q0, q1 - q0, c->col[side], c->d_mark,
                                c->stream));
    std::vector<uint8_t> mark((size_t)no);
    HIP_TRY(c, hipMemcpyAsync(mark.data(), c->d_mark, (size_t)no, hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // row 0 is always on the list: the history-space kernels load it for the
    // padding rows of a tile and multiply it by c_j = 0 (dual.hip), so it
    // must hold a rotated row, not what the allocation happened to contain
    // (a NaN there failed every pivot and sent the whole side to d-space)
    if (no > 0) mark[0] = 1;
    std::vector<QueueRec> list;
    for (int64_t r = 0; r < no; ++r)
      if (mark[r]) list.push_back(QueueRec{(int32_t)r, 0, 0});
    c->hrows_key[side][0] = q0;
    c->hrows_key[side][1] = q1;
    c->hrows_gen[side] = ++c->ver_counter;
    if ((double)list.size() > 0.7 * (double)no) {
      c->n_hrows[side] = -1;  // most of the table: one plain pass over it
    } else {
      rc = ensure(c, c->d_hrows[side], std::max<size_t>(list.size(), 1));
      if (rc) return rc;
      if (!list.empty())
        HIP_TRY(c, hipMemcpy(c->d_hrows[side], list.data(), sizeof(QueueRec) * list.size(),
                             hipMemcpyHostToDevice));
      c->n_hrows[side] = (int64_t)list.size();
    }
  }
  if (c->n_hrows[side] >= 0) {
    *rows = c->d_hrows[side];
    *nrows = c->n_hrows[side];
    *sub = c->hrows_gen[side];
  }
  return FRECSYS_OK;
}

// A Gramian of side g was just formed on c->stream: build its basis on
// stream5 now if the side that consumes it took the history-space path last
// time and will want it again.
static int maybe_start_eager(frecsys_ctx* c, int g) {
  const int consumer = 1 - g;
  if (!c->eager_on || c->dual_serial || !c->dual_on || c->Dp < 64 || c->dual_max_h <= 0 ||
      !c->dual_used[consumer] || c->eager_pending[g])
    return FRECSYS_OK;
  // the consumer's last row subset (its next solve checks it still applies)
  const bool subset = c->n_hrows[consumer] >= 0 && c->hrows_key[consumer][0] >= 0;
  const QueueRec* rows = subset ? c->d_hrows[consumer] : nullptr;
  const uint64_t sub = subset ? c->hrows_gen[consumer] : 0;
  if (c->basis_gram[g] == c->gram_ver[g] && c->xrot_emb[g] == c->emb_ver[g] &&
      c->xrot_gram[g] == c->gram_ver[g] && c->basis_mode[g] == c->want_mode[g] &&
      c->basis_mu[g] == c->want_mu[g] && c->basis_lam[g] == c->want_lam[g] &&
      (c->xrot_sub[g] == 0 || c->xrot_sub[g] == sub))
    return FRECSYS_OK;  // already current
  HIP_TRY(c, hipEventRecord(c->ev_pre5, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->stream5, c->ev_pre5, 0));
  int rc = prepare_basis(c, g, c->emb[g], c->stream5, c->want_mode[g], c->want_mu[g],
                         c->want_lam[g], rows, subset ? c->n_hrows[consumer] : 0, sub);
  if (rc) return rc;
  HIP_TRY(c, hipEventRecord(c->ev_eager[g], c->stream5));
  c->eager_pending[g] = true;
  return FRECSYS_OK;
}

// Row-range all-gather of a [rows x ld] float matrix (uneven per-rank
// counts): every rank broadcasts its own range in place.
int allgather_rows(frecsys_ctx* c, float* base, int side, int64_t ld) {
  if (!c->comm) return FRECSYS_OK;  // world 1 without RCCL, or external exchange: the caller's
  NCCL_TRY(c, ncclGroupStart());
  for (int r = 0; r < c->world; ++r) {
    const int64_t lo = c->bounds[side][r], hi = c->bounds[side][r + 1];
    const size_t cnt = (size_t)(hi - lo) * ld;
    if (cnt == 0) continue;
    float* p = base + lo * ld;
    NCCL_TRY(c, ncclBroadcast(p, p, cnt, ncclFloat, r, c->comm, c->stream));
  }
  NCCL_TRY(c, ncclGroupEnd());
  return FRECSYS_OK;
}

// The exchanges a sharded call makes inside itself, one code path for both
// transports: RCCL (a communicator) or the caller's callbacks
// (frecsys_set_transport).  Without either (world 1, or external exchange
// with no transport) a call does not exchange; the caller completes it.
bool in_call_exchange(const frecsys_ctx* c) { return c->world > 1 && (c->comm || c->has_transport); }

// All-gather of a per-row device table of `side` (ld floats per row).
int xchg_rows(frecsys_ctx* c, float* base, int side, int64_t ld) {
  if (c->comm) return allgather_rows(c, base, side, ld);
  if (!c->has_transport) return FRECSYS_OK;
  const int64_t n = c->n[side];
  std::vector<float> h((size_t)std::max<int64_t>(n * ld, 1));
  if (n) HIP_TRY(c, hipMemcpyAsync(h.data(), base, sizeof(float) * n * ld, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int64_t lo, hi;
  shard(c, side, &lo, &hi);
  if (c->transport.allgather_rows(c->transport.user, side, h.data(), n, ld, lo, hi) != 0)
    return fail(c, FRECSYS_ERR_RCCL, "transport: allgather_rows failed");
  if (n) HIP_TRY(c, hipMemcpyAsync(base, h.data(), sizeof(float) * n * ld, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

// In-place minimum over ranks of one device u64.
int xchg_min_u64(frecsys_ctx* c, unsigned long long* dval) {
  if (c->comm) {
    NCCL_TRY(c, ncclAllReduce(dval, dval, 1, ncclUint64, ncclMin, c->comm, c->stream));
    return FRECSYS_OK;
  }
  if (!c->has_transport) return FRECSYS_OK;
  uint64_t v = 0;
  HIP_TRY(c, hipMemcpyAsync(&v, dval, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->transport.allreduce_min_u64(c->transport.user, &v) != 0)
    return fail(c, FRECSYS_ERR_RCCL, "transport: allreduce_min_u64 failed");
  HIP_TRY(c, hipMemcpyAsync(dval, &v, sizeof(v), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

// Host -> device upload of a per-entity vector through a pinned staging
// buffer of its own (one per destination): a DMA the stream orders like a
// kernel, instead of a pageable-memory copy that the runtime stages itself
// (observed waiting for work queued on other streams).  Every call that
// uploads synchronises its stream before returning, so a staging buffer is
// never rewritten while its copy is in flight.
int upload(frecsys_ctx* c, UploadBuf& b, const float* host, size_t n) {
  int rc = ensure(c, b.dev, n);
  if (rc) return rc;
  HIP_TRY(c, b.stage.reserve(n));
  if (n) std::memcpy(b.stage.get(), host, sizeof(float) * n);
  HIP_TRY(c, hipMemcpyAsync(b.dev, b.stage.get(), sizeof(float) * n, hipMemcpyHostToDevice,
                            c->stream));
  return FRECSYS_OK;
}

// Event pair around one launch on any stream; resolved by flush_ktimers
// after the stream has been synchronised.
static hipEvent_t pool_event(frecsys_ctx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  c->events.emplace_back();
  (void)hipEventCreate(&c->events.back().h);
  return c->events.back();
}
size_t ktimer_begin(frecsys_ctx* c, const std::string& name, hipStream_t s) {
  frecsys_ctx::Pending p{name, pool_event(c), pool_event(c)};
  (void)hipEventRecord(p.a, s);
  c->pending.push_back(p);
  return c->pending.size() - 1;
}
void ktimer_end(frecsys_ctx* c, size_t i, hipStream_t s) {
  (void)hipEventRecord(c->pending[i].b, s);
}
void flush_ktimers(frecsys_ctx* c) {
  for (auto& p : c->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(p.b) == hipSuccess &&
        hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      Timer& t = c->timers[p.name];
      t.total_ms += ms;
      t.launches += 1;
    } else {
      (void)hipGetLastError();  // a timer that cannot be read is dropped, not left as the
                                // thread's last error for the next launch to report
    }
    c->event_pool.push_back(p.a);
    c->event_pool.push_back(p.b);
  }
  c->pending.clear();
}

}  // namespace frecsys_hip

namespace {

// Group slabs of [r's groups] broadcast from their owners (an all-gather
// with uneven counts, in place).
int allgather_groups(frecsys_ctx* c, float* gslabs, const GramPlan& pl) {
  if (!c->comm || pl.ngroup == 0) return FRECSYS_OK;
  NCCL_TRY(c, ncclGroupStart());
  for (int r = 0; r < c->world; ++r) {
    int lo, hi;
    gram_owned_groups(pl, c->world, r, &lo, &hi);
    if (hi <= lo) continue;
    float* p = gslabs + (size_t)lo * pl.slab_floats;
    NCCL_TRY(c, ncclBroadcast(p, p, (size_t)(hi - lo) * pl.slab_floats, ncclFloat, r, c->comm,
                              c->stream));
  }
  NCCL_TRY(c, ncclGroupEnd());
  return FRECSYS_OK;
}

// G = X^T diag(w) X over all rows of X (n rows) by the partition-
// independent plan (kernels.h GramPlan): this rank computes its own groups,
// the group slabs are all-gathered (with a communicator) and every rank sums
// them in group order.  Without a communicator at world > 1 (external
// exchange) the other ranks' slabs are zero: G is this rank's partial sum.
// `all_groups`: compute every group here (diagnostics on one rank).
int form_gramian(frecsys_ctx* c, int slot, const float* X, int64_t n, const float* dw, float* G,
                 bool all_groups) {
  const GramPlan pl = gram_plan(c->Dp, n);
  int g_lo = 0, g_hi = pl.ngroup;
  if (!all_groups) gram_owned_groups(pl, c->world, c->rank, &g_lo, &g_hi);
  int rc = ensure(c, c->d_partials, gram_leaf_floats(pl, g_lo, g_hi));
  if (rc) return rc;
  rc = ensure(c, c->d_gslabs[slot], std::max<size_t>((size_t)pl.ngroup * pl.slab_floats, 1));
  if (rc) return rc;
  if (!all_groups && c->world > 1 && !c->comm && pl.ngroup > 0)
    HIP_TRY(c, hipMemsetAsync(c->d_gslabs[slot], 0, sizeof(float) * pl.ngroup * pl.slab_floats,
                              c->stream));
  GramArgs g{};
  g.X = X;
  g.w = dw;
  g.partials = c->d_partials;
  g.gslabs = c->d_gslabs[slot];
  g.plan = pl;
  g.g_lo = g_lo;
  g.g_hi = g_hi;
  HIP_TRY(c, launch_gramian(c->Dp, g, c->stream));
  if (slot < 2 && g_hi > g_lo) {  // 2 N d^2 over the rows of the groups formed here
    const int64_t r0 = gram_group_leaf(pl, g_lo) * pl.rpl;
    const int64_t r1 = std::min<int64_t>(n, gram_group_leaf(pl, g_hi) * pl.rpl);
    const double rows = (double)(r1 - r0), dd = c->dim;
    add_work(c, "gramian", 2.0 * rows * dd * dd, rows * dd * 4.0, r1 - r0);
  }
  if (!all_groups && c->comm) {
    const size_t k = ktimer_begin(c, "gram_exchange", c->stream);
    rc = allgather_groups(c, c->d_gslabs[slot], pl);
    if (rc) return rc;
    ktimer_end(c, k, c->stream);
  }
  HIP_TRY(c, launch_gram_final(c->Dp, pl, c->d_gslabs[slot], G, c->stream));
  if (slot < 2) {
    c->gplan[slot] = pl;
    c->gram_own[slot][0] = g_lo;
    c->gram_own[slot][1] = g_hi;
  }
  return FRECSYS_OK;
}

// Restatement of libstdc++ std::normal_distribution<float>::operator()
// (Marsaglia polar; bits/random.tcc) over std::generate_canonical<float,24>
// of std::mt19937, with FMA contraction off so x*x + y*y rounds like the
// un-fused library code.  Drives the seeded init of init_matrix
// (recommender.h:61-67).
#pragma clang fp contract(off)
struct NormalF {
  bool saved_available = false;
  float saved = 0.f;
  static float canonical(std::mt19937& g) {
    float s = (float)g();
    float r = s / 4294967296.0f;
    if (r >= 1.0f) r = std::nextafter(1.0f, 0.0f);
    return r;
  }
  float operator()(std::mt19937& g, float mean, float stddev) {
    float ret;
    if (saved_available) {
      saved_available = false;
      ret = saved;
    } else {
      float x, y, r2;
      do {
        x = (float)((double)(2.0f * canonical(g)) - 1.0);
        y = (float)((double)(2.0f * canonical(g)) - 1.0);
        r2 = x * x + y * y;
      } while (r2 > 1.0 || r2 == 0.0);
      const float mult = std::sqrt(-2 * std::log(r2) / r2);
      saved = x * mult;
      saved_available = true;
      ret = y * mult;
    }
    return ret * stddev + mean;
  }
};

// n draws of a fresh NormalF (a new distribution per matrix,
// recommender.h:61-67) from g, bit-identical to calling it n times, in two
// passes: the polar method's accept / reject decisions need only the
// uniforms (a cheap sequential scan that advances g exactly as NormalF
// does), and the log / sqrt of each accepted pair are independent, so they
// run on threads.  2M x 1024 + 500K x 1024 draws: the serial loop's ~1 min
// becomes a few seconds.
void fill_normal(std::mt19937& g, float mean, float stddev, float* out, size_t n) {
  const size_t pairs = (n + 1) / 2;
  std::vector<float> px(pairs), py(pairs), pr(pairs);
  for (size_t p = 0; p < pairs; ++p) {
    float x, y, r2;
    do {
      x = (float)((double)(2.0f * NormalF::canonical(g)) - 1.0);
      y = (float)((double)(2.0f * NormalF::canonical(g)) - 1.0);
      r2 = x * x + y * y;
    } while (r2 > 1.0 || r2 == 0.0);
    px[p] = x;
    py[p] = y;
    pr[p] = r2;
  }
  auto work = [&](size_t lo, size_t hi) {
    for (size_t p = lo; p < hi; ++p) {
      const float r2 = pr[p];
      const float mult = std::sqrt(-2 * std::log(r2) / r2);
      const float first = py[p] * mult;   // returned first ...
      const float second = px[p] * mult;  // ... then the saved value
      out[2 * p] = first * stddev + mean;
      if (2 * p + 1 < n) out[2 * p + 1] = second * stddev + mean;
    }
  };
  const size_t nt = std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
  if (pairs < (size_t)1 << 16 || nt == 1) {
    work(0, pairs);
    return;
  }
  std::vector<std::thread> th;
  for (size_t t = 0; t < nt; ++t)
    th.emplace_back(work, pairs * t / nt, pairs * (t + 1) / nt);
  for (auto& t : th) t.join();
}
#pragma clang fp contract(on)

}  // namespace

extern "C" {

int32_t frecsys_padded_dim(int32_t dim) { return padded_dim(dim); }

int frecsys_device_count(int32_t* n) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess) {
    *n = 0;
    return fail(nullptr, FRECSYS_ERR_NO_DEVICE, hipGetErrorString(e));
  }
  *n = cnt;
  return FRECSYS_OK;
}

const char* frecsys_last_error(const frecsys_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_last_error.c_str();
}

int64_t frecsys_last_error_entity(const frecsys_ctx* ctx) { return ctx ? ctx->err_entity : -1; }

int frecsys_partition(int64_t n_rows, const int64_t* row_ptr, int32_t nparts, int64_t* bounds) {
  if (n_rows < 0 || nparts <= 0 || !row_ptr || !bounds)
    return fail(nullptr, FRECSYS_ERR_INVALID, "frecsys_partition: bad arguments");
  partition_rows(n_rows, row_ptr, nparts, bounds);
  return FRECSYS_OK;
}

int frecsys_gram_plan(int32_t dim, int64_t n_rows, int32_t world, int32_t rank,
                      int64_t* rows_per_leaf, int64_t* n_leaves, int32_t* n_groups,
                      int32_t* own_lo, int32_t* own_hi) {
  const int Dp = padded_dim(dim);
  if (Dp == 0 || n_rows < 0 || world <= 0 || rank < 0 || rank >= world)
    return fail(nullptr, FRECSYS_ERR_INVALID, "frecsys_gram_plan: bad arguments");
  const GramPlan pl = gram_plan(Dp, n_rows);
  int lo, hi;
  gram_owned_groups(pl, world, rank, &lo, &hi);
  if (rows_per_leaf) *rows_per_leaf = pl.rpl;
  if (n_leaves) *n_leaves = pl.nleaf;
  if (n_groups) *n_groups = pl.ngroup;
  if (own_lo) *own_lo = lo;
  if (own_hi) *own_hi = hi;
  return FRECSYS_OK;
}

int frecsys_ctx_create(const frecsys_config* cfg, frecsys_ctx** out) {
  if (!cfg || !out) return fail(nullptr, FRECSYS_ERR_INVALID, "null argument");
  *out = nullptr;
  const int Dp = padded_dim(cfg->dim);
  if (Dp == 0)
    return fail(nullptr, FRECSYS_ERR_UNSUPPORTED,
                "dim " + std::to_string(cfg->dim) + " not supported (1..1024 built)");
  if (cfg->n_users < 0 || cfg->n_items < 0)
    return fail(nullptr, FRECSYS_ERR_INVALID, "negative entity counts");
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0)
    return fail(nullptr, FRECSYS_ERR_NO_DEVICE, "no HIP device visible");
  auto* c = new frecsys_ctx();
  c->dim = cfg->dim;
  c->Dp = Dp;
  c->quirks = cfg->parity_quirks;
  c->n[0] = cfg->n_users;
  c->n[1] = cfg->n_items;
  if (cfg->device >= 0) {
    c->device = cfg->device;
  } else {
    (void)hipGetDevice(&c->device);
  }
  auto bail = [&](int rc) {
    g_last_error = c->err;
    frecsys_ctx_destroy(c);
    return rc;
  };
  if (hipSetDevice(c->device) != hipSuccess)
    return bail(fail(c, FRECSYS_ERR_NO_DEVICE, "hipSetDevice failed"));
  {  // the history-space chain (basis -> buckets) runs on the high-priority stream
    int lo_pri = 0, hi_pri = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri);
    if (hipStreamCreateWithPriority(&c->stream.h, hipStreamNonBlocking, hi_pri) != hipSuccess)
      return bail(fail(c, FRECSYS_ERR_HIP, "hipStreamCreate failed"));
  }
  if (hipEventCreate(&c->ev0.h) != hipSuccess || hipEventCreate(&c->ev1.h) != hipSuccess)
    return bail(fail(c, FRECSYS_ERR_HIP, "hipEventCreate failed"));
  // the second bucket lane / early builds at normal priority (high priority
  // measured no better)
  const int s3_pri = 0;
  if (hipStreamCreateWithFlags(&c->stream2.h, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithPriority(&c->stream3.h, hipStreamNonBlocking, s3_pri) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork.h, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join.h, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork3.h, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join3.h, hipEventDisableTiming) != hipSuccess)
    return bail(fail(c, FRECSYS_ERR_HIP, "hipStreamCreate failed (stream2/3)"));
  // the early basis builds share stream3 with the second bucket lane: with
  // GPU_MAX_HW_QUEUES = 4 a fifth stream shared a hardware queue with the
  // d-space stream, whose solve then waited (in FIFO order) for the whole
  // basis chain queued before it -- 0.5 ms per ML-20M epoch.  stream3 is idle
  // when a Gramian triggers an early build, and the buckets it runs later
  // need that basis anyway.
  c->stream5 = c->stream3.h;
  if (hipEventCreateWithFlags(&c->ev_pre5.h, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_eager[0].h, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_eager[1].h, hipEventDisableTiming) != hipSuccess)
    return bail(fail(c, FRECSYS_ERR_HIP, "hipEventCreate failed (early builds)"));
  if (const char* v = getenv("FRECSYS_DUAL")) c->dual_on = atoi(v);
  if (const char* v = getenv("FRECSYS_EAGER")) c->eager_on = atoi(v);
  if (const char* v = getenv("FRECSYS_CHOL_BASIS")) c->chol_basis_on = atoi(v);
  // d-space / history-space crossover: by flops h = d, but at Dp <= 256 the
  // d-space kernel overtakes the TH = 8 bucket (225 < h <= 256) in time (epoch
  // 15.6 -> 15.1 ms at the ML-20M shape, threshold sweep in DESIGN.md 3.2).
  // Dp = 1024: the wide bucket (256 < h_eff <= 512, dual.hip) as well (config
  // 5 epoch 1470 -> 1274 ms); Dp = 512: 256 (the wide bucket at 384 / 512
  // measured 124 / 129 ms against 115 at MSD).
  c->dual_max_h = Dp <= 256 ? 224 : Dp == 1024 ? 512 : 256;
  if (const char* v = getenv("FRECSYS_DUAL_MAX_H")) c->dual_max_h = atoi(v);
  if (const char* v = getenv("FRECSYS_DUAL_SERIAL")) c->dual_serial = atoi(v);
  if (const char* v = getenv("FRECSYS_CHOL_SCHED")) c->chol_sched = atoi(v) != 0;
  if (const char* v = getenv("FRECSYS_SPLIT_ROWS")) c->split_rows = atoi(v);
  if (const char* v = getenv("FRECSYS_DEBUG_SKIP")) {
#ifdef FRECSYS_ABLATION
    c->debug_skip = atoi(v);
#else
    // a release build has no ablation masks: refuse rather than silently
    // run the full work under a variable that claims to skip some
    if (atoi(v) != 0)
      return bail(fail(c, FRECSYS_ERR_INVALID,
                       "FRECSYS_DEBUG_SKIP needs a -DFRECSYS_ABLATION build of libfrecsys_hip.so"));
#endif
  }
  if (const char* v = getenv("FRECSYS_WIDE_WS_MB")) c->wide_ws_mb = std::max(1, atoi(v));
  if (const char* v = getenv("FRECSYS_WIDE_PRESPLIT")) c->wide_presplit = atoi(v) != 0;
  if (const char* v = getenv("FRECSYS_WS_FREE_CAP")) c->ws_free_cap = atoi(v) != 0;
  // the wide dims add the wide bucket (256 < h_eff <= 512, dual.hip)
  const int max_h_cap = Dp >= 512 ? kDualWideMaxH : 32 * kDualMaxTiles;
  c->dual_max_h = std::min(c->dual_max_h, max_h_cap);
  for (int t = 0; t < 3; ++t) c->dual_max_h_side[t] = c->dual_max_h;
  // Dp = 512, user side: 320.  That half-step is bound by its d-space stream
  // (MSD: 45 ms beside 29 of history space), and the wide bucket takes the
  // users with 256 < h_eff <= 320 off it: MSD 115.3 -> 114.1 ms (items: no
  // gain; DESIGN.md 3.8, profiles/r06/dual_max_h/)
  if (Dp == 512 && !getenv("FRECSYS_DUAL_MAX_H"))
    c->dual_max_h_side[FRECSYS_SIDE_USER] = std::min(320, max_h_cap);
  if (const char* v = getenv("FRECSYS_DUAL_MAX_H_USER"))
    c->dual_max_h_side[0] = std::min(atoi(v), max_h_cap);
  if (const char* v = getenv("FRECSYS_DUAL_MAX_H_ITEM"))
    c->dual_max_h_side[1] = std::min(atoi(v), max_h_cap);
  for (int s = 0; s < 2; ++s) {
    const size_t rows = (size_t)std::max<int64_t>(c->n[s], 1);
    if (c->emb[s].reserve(rows * Dp) != hipSuccess ||
        c->gram[s].reserve((size_t)Dp * Dp) != hipSuccess)
      return bail(fail(c, FRECSYS_ERR_HIP, "hipMalloc failed (embeddings)"));
    (void)hipMemsetAsync(c->emb[s], 0, sizeof(float) * rows * Dp, c->stream);
    (void)hipMemsetAsync(c->gram[s], 0, sizeof(float) * Dp * Dp, c->stream);
  }
  if (c->d_fail.reserve(1) != hipSuccess || c->d_counter.reserve(1) != hipSuccess ||
      c->d_events.reserve(4) != hipSuccess)
    return bail(fail(c, FRECSYS_ERR_HIP, "hipMalloc failed"));
  (void)hipMemsetAsync(c->d_events, 0, 4 * sizeof(unsigned int), c->stream);
  c->bounds[0] = {0, c->n[0]};
  c->bounds[1] = {0, c->n[1]};
  if (hipStreamSynchronize(c->stream) != hipSuccess)
    return bail(fail(c, FRECSYS_ERR_HIP, "stream sync failed"));
  *out = c;
  return FRECSYS_OK;
}

void frecsys_ctx_destroy(frecsys_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // every stream idle before the members go: the buffers first, then the
  // events and streams (stream5 is stream3)
  for (hipStream_t s : {c->stream5, c->stream.h, c->stream2.h})
    if (s) (void)hipStreamSynchronize(s);
  if (c->comm) ncclCommDestroy(c->comm);
  delete c;
}

int frecsys_comm_unique_id(uint8_t id[128]) {
  ncclUniqueId uid;
  ncclResult_t r = ncclGetUniqueId(&uid);
  if (r != ncclSuccess) return fail(nullptr, FRECSYS_ERR_RCCL, ncclGetErrorString(r));
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  std::memcpy(id, &uid, 128);
  return FRECSYS_OK;
}

int frecsys_comm_init(frecsys_ctx* c, int32_t world, int32_t rank, const uint8_t id[128]) {
  if (!c || world <= 0 || rank < 0 || rank >= world)
    return fail(c, FRECSYS_ERR_INVALID, "frecsys_comm_init: bad rank/world");
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->comm) {
    ncclCommDestroy(c->comm);
    c->comm = nullptr;
  }
  int rc = join_eager(c, 3, c->stream);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->gram_src[0] = c->gram_src[1] = 0;  // partials now sum over other shards
  c->world = world;
  c->rank = rank;
  if (id) {  // a communicator at every world size (world 1: the exchange path still runs)
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    NCCL_TRY(c, ncclCommInitRank(&c->comm, world, uid, rank));
  }
  refresh_bounds(c, 0);
  refresh_bounds(c, 1);
  c->order_stale[0] = c->order_stale[1] = true;
  return FRECSYS_OK;
}

int frecsys_shard_range(const frecsys_ctx* c, int32_t side, int64_t* lo, int64_t* hi) {
  if (!c || !valid_side(side) || !lo || !hi) return FRECSYS_ERR_INVALID;
  shard(c, side, lo, hi);
  return FRECSYS_OK;
}

int frecsys_load_csr(frecsys_ctx* c, int32_t side, int64_t n_rows, const int64_t* row_ptr,
                     const int32_t* col) {
  if (!c || !valid_side(side) || !row_ptr || n_rows < 0)
    return fail(c, FRECSYS_ERR_INVALID, "frecsys_load_csr: bad arguments");
  if (side < 2 && n_rows != c->n[side])
    return fail(c, FRECSYS_ERR_INVALID,
                "frecsys_load_csr: row count " + std::to_string(n_rows) + " != " +
                    std::to_string(c->n[side]));
  const int64_t nnz = row_ptr[n_rows] - row_ptr[0];
  if (row_ptr[0] != 0 || nnz < 0)
    return fail(c, FRECSYS_ERR_INVALID, "frecsys_load_csr: row_ptr must start at 0");
  if (side < 2) c->pp_order_all[side].clear();  // the residual order of a sharded pp_step
  const int other = side == 1 ? 0 : 1;
  const int64_t n_other = c->n[other];
  for (int64_t i = 0; i < n_rows; ++i)
    if (row_ptr[i + 1] < row_ptr[i])
      return fail(c, FRECSYS_ERR_INVALID, "frecsys_load_csr: row_ptr not monotone");
  for (int64_t k = 0; k < nnz; ++k)
    if (col[k] < 0 || col[k] >= n_other)  // assert(cp < item_embeddings.rows()), ials.h:116
      return fail(c, FRECSYS_ERR_INVALID,
                  "frecsys_load_csr: column id " + std::to_string(col[k]) + " out of range");
  HIP_TRY(c, hipSetDevice(c->device));
  {
    int rc = join_eager(c, 3, c->stream);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->gram_src[0] = c->gram_src[1] = 0;
  if (side == 2) emb_written(c, 2);
  HIP_TRY(c, renew(c->rp[side], (size_t)n_rows + 1));
  HIP_TRY(c, renew(c->col[side], (size_t)nnz));
  HIP_TRY(c, hipMemcpyAsync(c->rp[side], row_ptr, sizeof(int64_t) * (n_rows + 1),
                            hipMemcpyHostToDevice, c->stream));
  if (nnz)
    HIP_TRY(c, hipMemcpyAsync(c->col[side], col, sizeof(int32_t) * nnz, hipMemcpyHostToDevice,
                              c->stream));
  c->nnz[side] = nnz;
  c->order_stale[side] = true;
  if (side == 2) {
    c->host_rp_eval.assign(row_ptr, row_ptr + n_rows + 1);
    c->n[2] = n_rows;
    HIP_TRY(c, renew(c->emb[2], (size_t)std::max<int64_t>(n_rows, 1) * c->Dp));
    HIP_TRY(c, hipMemsetAsync(c->emb[2], 0, sizeof(float) * std::max<int64_t>(n_rows, 1) * c->Dp,
                              c->stream));
  } else {
    c->host_rp[side].assign(row_ptr, row_ptr + n_rows + 1);
    refresh_bounds(c, side);
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_set_embeddings(frecsys_ctx* c, int32_t side, const float* host, int64_t ld) {
  if (!c || !valid_side(side) || !host || ld < c->dim)
    return fail(c, FRECSYS_ERR_INVALID, "frecsys_set_embeddings: bad arguments");
  if (!c->emb[side]) return fail(c, FRECSYS_ERR_INVALID, "side has no embeddings yet");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = join_eager(c, 3, c->stream);
  if (rc) return rc;
  emb_written(c, side);
  const int64_t rows = c->n[side];
  HIP_TRY(c, hipMemsetAsync(c->emb[side], 0, sizeof(float) * std::max<int64_t>(rows, 1) * c->Dp,
                            c->stream));
  if (rows)
    HIP_TRY(c, hipMemcpy2DAsync(c->emb[side], sizeof(float) * c->Dp, host, sizeof(float) * ld,
                                sizeof(float) * c->dim, rows, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_get_embeddings(frecsys_ctx* c, int32_t side, float* host, int64_t ld) {
  if (!c || !valid_side(side) || !host || ld < c->dim)
    return fail(c, FRECSYS_ERR_INVALID, "frecsys_get_embeddings: bad arguments");
  if (!c->emb[side]) return fail(c, FRECSYS_ERR_INVALID, "side has no embeddings yet");
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t rows = c->n[side];
  if (rows)
    HIP_TRY(c, hipMemcpy2DAsync(host, sizeof(float) * ld, c->emb[side], sizeof(float) * c->Dp,
                                sizeof(float) * c->dim, rows, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_init_embeddings(frecsys_ctx* c, uint32_t seed, float stdev) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "null ctx");
  // ials.h:47-51: adjusted_stdev = stdev / sqrt(embedding_dim); one
  // generator, a new distribution per matrix (recommender.h:61-67).
  std::mt19937 gen{seed};
  const float adjusted = (float)((double)stdev / std::sqrt((double)c->dim));
  for (int s = 0; s < 2; ++s) {
    std::vector<float> h((size_t)c->n[s] * c->dim);
    fill_normal(gen, 0.0f, adjusted, h.data(), h.size());
    if (c->n[s]) {
      int rc = frecsys_set_embeddings(c, s, h.data(), c->dim);
      if (rc) return rc;
    }
  }
  return FRECSYS_OK;
}

int frecsys_snapshot(frecsys_ctx* c, int32_t side) {
  if (!c || side < 0 || side > 1) return fail(c, FRECSYS_ERR_INVALID, "snapshot: bad side");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = sizeof(float) * std::max<int64_t>(c->n[side], 1) * c->Dp;
  HIP_TRY(c, c->snap[side].reserve(bytes / sizeof(float)));
  HIP_TRY(c, hipMemcpyAsync(c->snap[side], c->emb[side], bytes, hipMemcpyDeviceToDevice,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_gramian(frecsys_ctx* c, int32_t side, const float* weights, int32_t from_snapshot,
                    float* host_out) {
  if (!c || side < 0 || side > 1) return fail(c, FRECSYS_ERR_INVALID, "gramian: bad side");
  if (from_snapshot && !c->snap[side])
    return fail(c, FRECSYS_ERR_INVALID, "gramian: no snapshot taken");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  const bool plain = !weights && !from_snapshot;
  if (plain && c->gram_src[side] != 0 && c->gram_src[side] == c->emb_ver[side]) {
    // the embeddings are unchanged since this Gramian was formed: the same
    // deterministic computation would write the same bits (on every rank)
    if (host_out)
      HIP_TRY(c, hipMemcpy2DAsync(host_out, sizeof(float) * c->dim, c->gram[side],
                                  sizeof(float) * c->Dp, sizeof(float) * c->dim, c->dim,
                                  hipMemcpyDeviceToHost, c->stream));
    rc = maybe_start_eager(c, side);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FRECSYS_OK;
  }
  rc = join_eager(c, 1 << side, c->stream);  // an early basis build still reading this G
  if (rc) return rc;
  const float* dw = nullptr;
  if (weights) {
    rc = upload(c, c->d_gram_w, weights, (size_t)c->n[side]);
    if (rc) return rc;
    dw = c->d_gram_w.dev;
  }
  {
    ScopedTimer t(c, "gramian");
    rc = form_gramian(c, side, from_snapshot ? c->snap[side] : c->emb[side], c->n[side], dw,
                      c->gram[side], false);
    if (rc) return rc;
    t.stop();
  }
  c->gram_ver[side] = ++c->ver_counter;
  c->gram_src[side] = plain ? c->emb_ver[side] : 0;
  if (host_out)
    HIP_TRY(c, hipMemcpy2DAsync(host_out, sizeof(float) * c->dim, c->gram[side],
                                sizeof(float) * c->Dp, sizeof(float) * c->dim, c->dim,
                                hipMemcpyDeviceToHost, c->stream));
  rc = maybe_start_eager(c, side);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  flush_ktimers(c);
  return FRECSYS_OK;
}

int frecsys_get_gramian(frecsys_ctx* c, int32_t side, float* host, int64_t ld) {
  if (!c || side < 0 || side > 1 || !host || ld < c->dim)
    return fail(c, FRECSYS_ERR_INVALID, "get_gramian: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy2DAsync(host, sizeof(float) * ld, c->gram[side], sizeof(float) * c->Dp,
                              sizeof(float) * c->dim, c->dim, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_gram_groups(const frecsys_ctx* c, int32_t side, int32_t* n_groups, int32_t* own_lo,
                        int32_t* own_hi, int64_t* floats_per_group) {
  if (!c || side < 0 || side > 1) return FRECSYS_ERR_INVALID;
  const GramPlan pl = gram_plan(c->Dp, c->n[side]);
  int lo, hi;
  gram_owned_groups(pl, c->world, c->rank, &lo, &hi);
  if (n_groups) *n_groups = pl.ngroup;
  if (own_lo) *own_lo = lo;
  if (own_hi) *own_hi = hi;
  if (floats_per_group) *floats_per_group = (int64_t)pl.slab_floats;
  return FRECSYS_OK;
}

int frecsys_get_gram_groups(frecsys_ctx* c, int32_t side, float* host) {
  if (!c || side < 0 || side > 1 || !host)
    return fail(c, FRECSYS_ERR_INVALID, "get_gram_groups: bad arguments");
  const GramPlan& pl = c->gplan[side];
  if (!c->d_gslabs[side] || pl.n != c->n[side])
    return fail(c, FRECSYS_ERR_INVALID, "get_gram_groups: no Gramian formed for side");
  HIP_TRY(c, hipSetDevice(c->device));
  if (pl.ngroup)
    HIP_TRY(c, hipMemcpyAsync(host, c->d_gslabs[side], sizeof(float) * pl.ngroup * pl.slab_floats,
                              hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_set_gram_groups(frecsys_ctx* c, int32_t side, const float* host) {
  if (!c || side < 0 || side > 1 || !host)
    return fail(c, FRECSYS_ERR_INVALID, "set_gram_groups: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = join_eager(c, 1 << side, c->stream);
  if (rc) return rc;
  const GramPlan pl = gram_plan(c->Dp, c->n[side]);
  rc = ensure(c, c->d_gslabs[side], std::max<size_t>((size_t)pl.ngroup * pl.slab_floats, 1));
  if (rc) return rc;
  if (pl.ngroup)
    HIP_TRY(c, hipMemcpyAsync(c->d_gslabs[side], host, sizeof(float) * pl.ngroup * pl.slab_floats,
                              hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_gram_final(c->Dp, pl, c->d_gslabs[side], c->gram[side], c->stream));
  c->gplan[side] = pl;
  c->gram_ver[side] = ++c->ver_counter;
  c->gram_src[side] = 0;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_comm_world(const frecsys_ctx* c, int32_t* world, int32_t* rank, int32_t* comm_ranks) {
  if (!c) return FRECSYS_ERR_INVALID;
  if (world) *world = c->world;
  if (rank) *rank = c->rank;
  if (comm_ranks) {
    int n = 0;
    if (c->comm && ncclCommCount(c->comm, &n) != ncclSuccess) return FRECSYS_ERR_RCCL;
    *comm_ranks = n;  // 0: no communicator
  }
  return FRECSYS_OK;
}

int frecsys_set_gramian(frecsys_ctx* c, int32_t side, const float* host, int64_t ld) {
  if (!c || side < 0 || side > 1 || !host || ld < c->dim)
    return fail(c, FRECSYS_ERR_INVALID, "set_gramian: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = join_eager(c, 1 << side, c->stream);
  if (rc) return rc;
  c->gram_ver[side] = ++c->ver_counter;
  c->gram_src[side] = 0;
  HIP_TRY(c, hipMemsetAsync(c->gram[side], 0, sizeof(float) * c->Dp * c->Dp, c->stream));
  HIP_TRY(c, hipMemcpy2DAsync(c->gram[side], sizeof(float) * c->Dp, host, sizeof(float) * ld,
                              sizeof(float) * c->dim, c->dim, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_user_loss(frecsys_ctx* c, int32_t side, float beta, int32_t half, float* host_out) {
  if (!c || (side != 0 && side != 2)) return fail(c, FRECSYS_ERR_INVALID, "loss: bad side");
  if (!c->rp[side]) return fail(c, FRECSYS_ERR_INVALID, "loss: no CSR loaded");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t rows = (size_t)c->n[side];
  const bool fresh = c->d_loss.cap() < rows || !c->d_loss;
  int rc = ensure(c, c->d_loss, rows);
  if (rc) return rc;
  // external exchange (world > 1, no communicator): nothing gathers the
  // other ranks' rows, so they read 0, not what an earlier EVAL call left
  if (fresh || side == 2 || (c->world > 1 && !c->comm))
    HIP_TRY(c, hipMemsetAsync(c->d_loss, 0, sizeof(float) * std::max<size_t>(rows, 1), c->stream));
  int64_t lo, hi;
  shard(c, side, &lo, &hi);
  // Dp = 64..256: u^T G u by the rotation kernel (column-block partials; it
  // measured faster than quad_kernel's f32 MFMA, which keeps the other widths)
  const bool qr = !wide_dim(c->Dp) && c->Dp >= 64 && c->Dp % 32 == 0;
  rc = ensure(c, c->d_quad, std::max<size_t>(wide_dim(c->Dp) ? wide_quad_floats(c->Dp, hi - lo)
                               : qr ? (size_t)rotate_quad_parts(c->Dp) * (size_t)(hi - lo)
                                    : rows,
                               1));
  if (rc) return rc;
  LossArgs a{};
  a.quad = c->d_quad;
  a.quad_parts = qr ? rotate_quad_parts(c->Dp) : 0;
  if (wide_dim(c->Dp) || qr) {
    HIP_TRY(c, c->gsplit.reserve(basis_split_bytes(c->Dp)));
    a.gsplit = c->gsplit;
  }
  a.row_ptr = c->rp[side];
  a.col = c->col[side];
  a.row_lo = lo;
  a.n_rows = hi - lo;
  a.U = c->emb[side];
  a.V = c->emb[1];
  a.G = c->gram[1];
  a.beta = beta;
  a.half = half;
  a.out = c->d_loss;
  {
    // user_loss: both kernels; user_loss.gather: the gather kernel alone (its
    // own rate for the loss_gather roofline)
    frecsys_ctx::Pending g{"user_loss.gather", pool_event(c), pool_event(c)};
    // (no launch on an empty shard: an event nobody records must not be timed)
    a.ev_gather = (c->Dp > 16 && a.n_rows > 0) ? g.a : nullptr;
    ScopedTimer t(c, "user_loss");
    HIP_TRY(c, launch_user_loss(c->Dp, a, c->stream));
    if (a.ev_gather) {
      (void)hipEventRecord(g.b, c->stream);
      c->pending.push_back(g);
    } else {
      c->event_pool.push_back(g.a);
      c->event_pool.push_back(g.b);
    }
    t.stop();
    flush_ktimers(c);
  }
  if (side == 0) {  // gather of the item rows + u^T G u: SURVEY 8(d) bytes with a 1-float output
    const std::vector<int64_t>& rp = c->host_rp[0];
    const double nnz = rp.empty() ? 0.0 : (double)(rp[hi] - rp[lo]), n = (double)(hi - lo);
    const double dd = c->dim;
    add_work(c, "user_loss", 2.0 * nnz * dd + 2.0 * n * dd * dd,
             nnz * dd * 4.0 + nnz * 4.0 + (n + 1.0) * 8.0 + n * 4.0, hi - lo);
  }
  if (host_out) {
    if (side == 0 && (c->world > 1 || c->comm)) {
      rc = allgather_rows(c, c->d_loss, 0, 1);
      if (rc) return rc;
    }
    if (rows)
      HIP_TRY(c, hipMemcpyAsync(host_out, c->d_loss, sizeof(float) * rows, hipMemcpyDeviceToHost,
                                c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_eval_topk(frecsys_ctx* c, int32_t k, int32_t* topk) {
  if (!c || !topk) return fail(c, FRECSYS_ERR_INVALID, "eval_topk: bad arguments");
  if (!c->rp[2] || !c->emb[2]) return fail(c, FRECSYS_ERR_INVALID, "eval_topk: no EVAL side loaded");
  const int64_t n = c->n[2], m = c->n[1];
  if (k < 1 || k > 1024 || k > m)
    return fail(c, FRECSYS_ERR_INVALID, "eval_topk: k must be in [1, min(1024, items)]");
  if (n == 0) return FRECSYS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  // scores in batches of rows bounded to 1 GiB of workspace
  const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)1 << 28) / m));
  int rc = ensure(c, c->d_scores, (size_t)nb * m);
  if (rc) return rc;
  rc = ensure(c, c->d_topk, (size_t)n * k);
  if (rc) return rc;
  {
    ScopedTimer t(c, "eval_topk");
    for (int64_t r0 = 0; r0 < n; r0 += nb) {
      const int64_t cnt = std::min(nb, n - r0);
      HIP_TRY(c, launch_eval_topk(c->emb[2], r0, cnt, c->emb[1], m, c->Dp, c->rp[2], c->col[2], k,
                                  c->d_scores, c->d_topk + r0 * k, c->stream));
    }
    t.stop();
  }
  HIP_TRY(c, hipMemcpyAsync(topk, c->d_topk, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_set_transport(frecsys_ctx* c, const frecsys_transport* t) {
  if (!c) return FRECSYS_ERR_INVALID;
  if (t && (!t->allgather_rows || !t->allreduce_min_u64))
    return fail(c, FRECSYS_ERR_INVALID, "set_transport: every callback is required");
  if (c->pp_old_side != -1)
    return fail(c, FRECSYS_ERR_INVALID, "set_transport: pp_sync pending");
  c->has_transport = t != nullptr;
  c->transport = t ? *t : frecsys_transport{};
  return FRECSYS_OK;
}

int frecsys_train_stats(frecsys_ctx* c, double* observed, double* unobserved,
                        float* user_norm2, float* item_norm2) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "train_stats: null ctx");
  if (observed && !c->rp[0]) return fail(c, FRECSYS_ERR_INVALID, "train_stats: no USER CSR");
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t nu = c->n[0], ni = c->n[1];
  const int Dp = c->Dp;
  int rc = ensure(c, c->d_rows, (size_t)std::max<int64_t>(std::max(nu, ni), 1));
  if (rc) return rc;
  ScopedTimer t(c, "train_stats");
  if (observed) {
    LossArgs a{};
    a.row_ptr = c->rp[0];
    a.col = c->col[0];
    a.row_lo = 0;
    a.n_rows = nu;
    a.U = c->emb[0];
    a.V = c->emb[1];
    a.G = c->gram[1];
    a.out = c->d_rows;
    a.raw = 1;
    HIP_TRY(c, hipMemsetAsync(c->d_rows, 0, sizeof(float) * std::max<int64_t>(nu, 1), c->stream));
    HIP_TRY(c, launch_user_loss(Dp, a, c->stream));
    std::vector<float> h((size_t)nu);
    if (nu)
      HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_rows, sizeof(float) * nu, hipMemcpyDeviceToHost,
                                c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double s = 0.0;
    for (float v : h) s += (double)v;
    *observed = s;
  }
  if (unobserved) {
    rc = ensure(c, c->d_gstat, (size_t)2 * Dp * Dp);
    if (rc) return rc;
    rc = ensure(c, c->d_dot, 1);
    if (rc) return rc;
    for (int s = 0; s < 2; ++s) {
      rc = form_gramian(c, 2, c->emb[s], c->n[s], nullptr, c->d_gstat + (size_t)s * Dp * Dp, true);
      if (rc) return rc;
    }
    HIP_TRY(c, launch_gram_dot(c->d_gstat, c->d_gstat + (size_t)Dp * Dp, Dp, c->d_dot, c->stream));
    HIP_TRY(c, hipMemcpyAsync(unobserved, c->d_dot, sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
  }
  for (int s = 0; s < 2; ++s) {
    float* host = s == 0 ? user_norm2 : item_norm2;
    if (!host || c->n[s] == 0) continue;
    HIP_TRY(c, launch_row_norm2(c->emb[s], c->n[s], Dp, c->d_rows, c->stream));
    HIP_TRY(c, hipMemcpyAsync(host, c->d_rows, sizeof(float) * c->n[s], hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  t.stop();
  return FRECSYS_OK;
}

int frecsys_synchronize(frecsys_ctx* c) {
  if (!c) return FRECSYS_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream5));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_release_workspaces(frecsys_ctx* c) {
  if (!c) return FRECSYS_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream5));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, c->wide_ws.release());
  HIP_TRY(c, c->wide_xs.release());
  HIP_TRY(c, c->d_slabs.release());
  HIP_TRY(c, c->dw_zs.release());
  HIP_TRY(c, c->dw_slots.release());
  HIP_TRY(c, c->dw_z.release());
  HIP_TRY(c, c->d_rec.release());
  HIP_TRY(c, c->d_sim_inv.release());
  HIP_TRY(c, c->d_samp_ids.release());
  HIP_TRY(c, c->d_ts_img.release());
  HIP_TRY(c, c->d_ts_norm.release());
  HIP_TRY(c, c->d_ts_stats.release());
  return FRECSYS_OK;
}

int frecsys_timing(const frecsys_ctx* c, const char* what, double* total_ms, int64_t* launches) {
  if (!c || !what) return FRECSYS_ERR_INVALID;
  auto it = c->timers.find(what);
  if (total_ms) *total_ms = it == c->timers.end() ? 0.0 : it->second.total_ms;
  if (launches) *launches = it == c->timers.end() ? 0 : it->second.launches;
  return FRECSYS_OK;
}

int frecsys_work(const frecsys_ctx* c, const char* what, double* flops, double* bytes,
                 int64_t* entities, int64_t* launches) {
  if (!c || !what) return FRECSYS_ERR_INVALID;
  auto it = c->work.find(what);
  const Work w = it == c->work.end() ? Work{} : it->second;
  if (flops) *flops = w.flops;
  if (bytes) *bytes = w.bytes;
  if (entities) *entities = w.entities;
  if (launches) *launches = w.launches;
  return FRECSYS_OK;
}

int frecsys_debug_diag_factor(frecsys_ctx* c, int32_t blocked, int32_t n_tiles, const float* a,
                              float* linv, int32_t* ok) {
  if (!c || n_tiles < 0 || (n_tiles && (!a || !linv || !ok)))
    return fail(c, FRECSYS_ERR_INVALID, "debug_diag_factor: bad arguments");
  if (n_tiles == 0) return FRECSYS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf<float> dA, dL;
  DevBuf<int> dok;
  const size_t bytes = sizeof(float) * 1024 * (size_t)n_tiles;
  HIP_TRY(c, dA.reserve((size_t)1024 * n_tiles));
  HIP_TRY(c, dL.reserve((size_t)1024 * n_tiles));
  HIP_TRY(c, dok.reserve((size_t)n_tiles));
  HIP_TRY(c, hipMemcpyAsync(dA, a, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_debug_diag(dA, dL, dok, n_tiles, blocked ? 1 : 0, c->stream));
  HIP_TRY(c, hipMemcpyAsync(linv, dL, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(ok, dok, sizeof(int) * (size_t)n_tiles, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_debug_basis(frecsys_ctx* c, int32_t side, float* q, float* diag, float* sub) {
  if (!c || side < 0 || side > 1 || !q || !diag || !sub)
    return fail(c, FRECSYS_ERR_INVALID, "debug_basis: bad arguments");
  if (c->Dp < 64) return fail(c, FRECSYS_ERR_UNSUPPORTED, "debug_basis: Dp < 64");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = prepare_basis(c, side, c->emb[side], c->stream);
  if (rc) return rc;
  const size_t Dp = (size_t)c->Dp;
  HIP_TRY(c, hipMemcpyAsync(q, c->q[side], sizeof(float) * Dp * Dp, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipMemcpyAsync(diag, c->tri[side], sizeof(float) * Dp, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipMemcpyAsync(sub, c->tri[side] + Dp, sizeof(float) * Dp, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int32_t frecsys_history_space_max_h(const frecsys_ctx* c) {
  return c && c->dual_on && c->Dp >= 64 ? c->dual_max_h : 0;
}

int32_t frecsys_history_space_max_h_side(const frecsys_ctx* c, int32_t side) {
  if (!c || !c->dual_on || c->Dp < 64 || (side != FRECSYS_SIDE_USER && side != FRECSYS_SIDE_ITEM))
    return 0;
  return c->dual_max_h_side[side];
}

int frecsys_counter(frecsys_ctx* c, const char* what, int64_t* value) {
  if (!c || !what || !value) return fail(c, FRECSYS_ERR_INVALID, "counter: bad arguments");
  if (!strcmp(what, "hspace_reruns")) {
    *value = c->hspace_reruns;
    return FRECSYS_OK;
  }
  if (!strcmp(what, "ws_shrinks")) {
    *value = c->ws_shrinks;
    return FRECSYS_OK;
  }
  if (!strcmp(what, "cg_iterations")) {
    *value = c->cg_iterations;
    return FRECSYS_OK;
  }
  if (!strcmp(what, "cg_unconverged")) {
    *value = c->cg_unconverged;
    return FRECSYS_OK;
  }
  if (!strcmp(what, "recommend_splits")) {
    *value = c->rec_splits;
    return FRECSYS_OK;
  }
  if (!strcmp(what, "two_stage_certified")) {
    *value = c->ts_certified;
    return FRECSYS_OK;
  }
  if (!strcmp(what, "two_stage_fallback_rows")) {
    *value = c->ts_fallback_rows;
    return FRECSYS_OK;
  }
  if (!strcmp(what, "live_device_bytes")) {  // of the process, not of this context
    *value = live_device_bytes().load();
    return FRECSYS_OK;
  }
  if (!strcmp(what, "tagged_timeouts")) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream5));
    unsigned ev[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(ev, c->d_events, sizeof(ev), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *value = (int64_t)ev[0];
    return FRECSYS_OK;
  }
  return fail(c, FRECSYS_ERR_INVALID, std::string("counter: unknown counter ") + what);
}

int frecsys_snapshot_residual(frecsys_ctx* c, int32_t side, double* sq) {
  if (!c || side < 0 || side > 1 || !sq) return fail(c, FRECSYS_ERR_INVALID, "snapshot_residual: bad arguments");
  if (!c->snap[side]) return fail(c, FRECSYS_ERR_INVALID, "snapshot_residual: no snapshot taken");
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t n = c->n[side];
  int rc = ensure(c, c->d_rows, (size_t)std::max<int64_t>(n, 1));
  if (rc) return rc;
  *sq = 0.0;
  if (n == 0) return FRECSYS_OK;
  HIP_TRY(c, launch_row_diff2(c->emb[side], c->snap[side], n, c->Dp, c->d_rows, c->stream));
  std::vector<float> h((size_t)n);
  HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_rows, sizeof(float) * n, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  double s = 0.0;
  for (float v : h) s += (double)v;
  *sq = s;
  return FRECSYS_OK;
}

int frecsys_timing_reset(frecsys_ctx* c) {
  if (!c) return FRECSYS_ERR_INVALID;
  c->timers.clear();
  c->work.clear();
  return FRECSYS_OK;
}

}  // extern "C"
