// train.hip -- host side of the training calls of the C-ABI
// (include/frecsys_hip.h): frecsys_solve_side, frecsys_solve_side_cg,
// frecsys_cg_iterations and the iALS++ block step (frecsys_pp_*).  No kernels
// here: solve.hip, wide.hip, wide_syrk.hip, dual.hip, spectral.hip, cg.hip and
// pp.hip hold them (kernels.h).  The context, the queue, the basis and the
// exchanges are capi.hip's (ctx.h).  solve_side, near the end, lists the
// stages of frecsys_solve_side.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ctx.h"
#include "wide.h"

namespace {

const char* const kSolveNames[3] = {"solve_user", "solve_item", "solve_eval"};

bool is_vkind(int kind) { return kind == FRECSYS_KIND_WEIGHTED_V || kind == FRECSYS_KIND_CVAR_GRAD_V; }
bool is_ukind(int kind) { return kind == FRECSYS_KIND_WEIGHTED_U || kind == FRECSYS_KIND_CVAR_GRAD_U; }
bool is_grad(int kind) { return kind == FRECSYS_KIND_CVAR_GRAD_U || kind == FRECSYS_KIND_CVAR_GRAD_V; }

// SURVEY 8(d) per entity of h assembly rows at dim d: d-space SYRK
// h d (d+1) and LLT d^3/3 + 2 d^2 flops; gather bytes h d 4 (rows) + h 4
// (ids) + 8 (row offset) + d 4 (the solution written).
// (SYRK and gather are linear in h: summed from the queue prefix sums,
// heff_sums.)
double dspace_solve_flops(double d) { return d * d * d / 3.0 + 2.0 * d * d; }

// FRECSYS_DUAL_PROF diagnostics: cycle counters the solve kernels fill.
bool dual_prof_on() {
  static const bool on = getenv("FRECSYS_DUAL_PROF") != nullptr;
  return on;
}
// The counters of one kernel family (n words, zeroed when first allocated);
// nullptr when the diagnostics are off.
int prof_counters(frecsys_ctx* c, DevBuf<unsigned long long>& buf, size_t n,
                  unsigned long long** out) {
  *out = nullptr;
  if (!dual_prof_on()) return FRECSYS_OK;
  if (!buf) {
    HIP_TRY(c, buf.reserve(n));
    HIP_TRY(c, hipMemset(buf, 0, sizeof(unsigned long long) * n));
  }
  *out = buf.get();
  return FRECSYS_OK;
}
// ... read into out[n] and zeroed for the next launch (the caller has
// synchronised the stream that filled them).
int prof_readback(frecsys_ctx* c, DevBuf<unsigned long long>& buf, size_t n,
                  unsigned long long* out) {
  HIP_TRY(c, hipMemcpy(out, buf, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemset(buf, 0, sizeof(unsigned long long) * n));
  return FRECSYS_OK;
}

// First position of side's queue with h_eff <= lim (the queue is sorted by
// decreasing history and h_eff is monotone in h).
int64_t first_le(const frecsys_ctx* c, int side, bool vq, int64_t lim) {
  const std::vector<int32_t>& hs = c->order_h[side];
  return (int64_t)(std::partition_point(hs.begin(), hs.end(), [&](int32_t h) {
                     return queue_heff(c->quirks, vq, h) > lim;
                   }) - hs.begin());
}

// Long-history split of the d-space queue prefix [0, n) of `side`: entities
// with more than 2*C assembly rows get their SYRK cut into C-row slabs done by
// separate workgroups (launch_split_syrk / wide_syrk2_kernel<2>) before the
// solve; at most max_slabs slabs of slab_floats each (longest entities first;
// shrink: fewer when their allocation fails -- only where the split does not
// change the sums' order, the wide dims).
int plan_split(frecsys_ctx* c, int side, int64_t n, bool vq, SolveArgs* a, int64_t C,
               size_t slab_floats, int64_t max_slabs, hipStream_t s, bool shrink = false) {
  const std::vector<int32_t>& hs = c->order_h[side];
  a->split = nullptr;
  a->n_split = 0;
  a->slabs = nullptr;
  a->work = nullptr;
  a->n_work = 0;
  if (c->split_rows <= 0 || C <= 0 || c->Dp < 32) return FRECSYS_OK;
  int32_t slab = 0;
  bool cut = false;
  while (true) {
    c->h_split.clear();
    c->h_work.clear();
    slab = 0;
    for (int64_t i = 0; i < n && queue_heff(c->quirks, vq, hs[i]) > 2 * C; ++i) {
      const int64_t ne = queue_heff(c->quirks, vq, hs[i]);
      if (slab + (ne + C - 1) / C > max_slabs) break;
      const int32_t first = slab;
      for (int64_t k = 0; k < ne; k += C)
        c->h_work.push_back(SplitWork{(int32_t)i, (int32_t)k, (int32_t)std::min(ne, k + C), slab++});
      c->h_split.push_back(int2{first, slab - first});
    }
    if (c->h_split.empty()) return FRECSYS_OK;
    if (!shrink) {
      int rc = ensure(c, c->d_slabs, (size_t)slab * slab_floats);
      if (rc) return rc;
      break;
    }
    // the wide dims (split and unsplit SYRKs are bit-identical there): fewer
    // slabs when the allocation fails
    bool oom = false;
    int rc = try_ensure(c, c->d_slabs, (size_t)slab * slab_floats, &oom);
    if (rc) return rc;
    if (!oom) {  // as ensure_batch: a cut allocation leaves kRuntimeHeadroom free
      if (!cut || slab <= 1 || !below_headroom()) break;
      HIP_TRY(c, c->d_slabs.release());
    }
    ++c->ws_shrinks;
    max_slabs = slab / 2;
    cut = true;
  }
  int rc = ensure(c, c->d_split, c->h_split.size());
  if (rc) return rc;
  rc = ensure(c, c->d_work, c->h_work.size());
  if (rc) return rc;
  // on the solve's own stream: a blocking hipMemcpy went through a queue that
  // could be FIFO-behind the basis chain, holding the d-space launch back
  // (h_split / h_work live in the context until the next call, after the
  // stream has been synchronised)
  HIP_TRY(c, hipMemcpyAsync(c->d_split, c->h_split.data(), sizeof(int2) * c->h_split.size(),
                            hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(c->d_work, c->h_work.data(), sizeof(SplitWork) * c->h_work.size(),
                            hipMemcpyHostToDevice, s));
  a->split = c->d_split;
  a->n_split = (int64_t)c->h_split.size();
  a->slabs = c->d_slabs;
  a->work = c->d_work;
  a->n_work = (int64_t)c->h_work.size();
  return FRECSYS_OK;
}

// The d-space solve of the queue prefix ap.order[0..ap.n_rows) at Dp = 512 /
// 1024: the HBM-workspace batches of wide.hip.
int launch_dspace_wide(frecsys_ctx* c, int side, SolveArgs ap, hipStream_t s,
                       const std::string& pre, bool can_split) {
  const bool vq = is_vkind(ap.kind);
  const size_t slot = wide_slot_floats(c->Dp);
  const int64_t budget =
      (int64_t)(ws_budget(c, c->wide_ws.cap() * sizeof(float)) / (slot * sizeof(float)));
  int64_t batch = std::max<int64_t>(1, std::min<int64_t>(ap.n_rows, budget));
  int rc = ensure_batch(c, c->wide_ws, slot, &batch);
  if (rc) return rc;
  if (can_split) {  // long histories of the first batch cut into slabs (a budget of their own)
    const size_t sf = wide_slab_floats(c->Dp);
    // (an empty shard has an empty queue but still a batch of one slot)
    rc = plan_split(c, side, std::min<int64_t>(batch, ap.n_rows), vq, &ap, wide_slab_rows(), sf,
                    (int64_t)(ws_budget(c, c->d_slabs.cap() * sizeof(float)) / (sf * sizeof(float))),
                    s, true);
    if (rc) return rc;
  }
  rc = prof_counters(c, c->w_prof, 16, &ap.prof);
  if (rc) return rc;
  char* xs = nullptr;
  if (c->wide_presplit && ap.n_rows > 0) {
    // no room for the table: the register-staged SYRK (bit-identical)
    bool oom = false;
    rc = try_ensure(c, c->wide_xs, wide_xsplit_bytes(c->Dp, ap.n_other), &oom);
    if (rc) return rc;
    if (oom) ++c->ws_shrinks;
    xs = c->wide_xs;
  }
  const size_t k = ktimer_begin(c, pre + ".dspace", s);
  HIP_TRY(c, launch_wide_solve(c->Dp, ap, c->wide_ws, batch, s, xs));
  ktimer_end(c, k, s);
  if (ap.prof) {  // diagnostics (ablation builds): wide SYRK cycles per chunk and phase
    unsigned long long hp[16];
    HIP_TRY(c, hipStreamSynchronize(s));
    rc = prof_readback(c, c->w_prof, 16, hp);
    if (rc) return rc;
    for (int pt = 0; pt < 2; ++pt)
      for (int wv = 0; wv < 2; ++wv) {
        const unsigned long long* q = hp + 8 * pt + 4 * wv;
        const double n = (double)std::max<unsigned long long>(q[3], 1);
        fprintf(stderr, "[wide-prof] %s %s wave %d chunks %llu cycles/chunk: mfma+stage %.0f "
                "ring+loads %.0f barrier %.0f\n", pre.c_str(), pt ? "diag" : "offdiag",
                wv ? 7 : 0, q[3], q[0] / n, q[1] / n, q[2] / n);
      }
  }
  // SURVEY 8(d) per entity: dspace_syrk_flops + dspace_solve_flops, gather_bytes
  // (empty histories untouched); both linear in h, so from the prefix sums
  const double d = c->dim;
  const HeffSums hsum = heff_sums(c, side, vq, 0, ap.n_rows);
  add_work(c, pre + ".dspace", d * (d + 1.0) * hsum.h1 + hsum.nz * dspace_solve_flops(d),
           (d * 4.0 + 4.0) * hsum.h1 + hsum.nz * (8.0 + d * 4.0), hsum.nz);  // one timed call
  return FRECSYS_OK;
}

// ... and up to Dp = 256: the tiled one-workgroup-per-entity kernels, long
// histories split.  aux (optional): an idle stream for the long histories'
// slabs and then their entities' solves, so the slabs run beside the other
// entities' solve instead of before it (s waits for aux at the end).
int launch_dspace_tiled(frecsys_ctx* c, int side, SolveArgs ap, hipStream_t s,
                        const std::string& pre, bool can_split, hipStream_t aux) {
  const bool vq = is_vkind(ap.kind);
  int rc = FRECSYS_OK;
  if (can_split) {
    rc = plan_split(c, side, ap.n_rows, vq, &ap, c->split_rows, split_slab_floats(c->Dp),
                    INT64_MAX, s);
    if (rc) return rc;
  }
  const bool side_split = ap.n_work > 0 && aux != nullptr;
  if (side_split) {
    // slabs, then the split entities' solves (they start from the slabs) on
    // aux; the other entities on s meanwhile
    HIP_TRY(c, hipEventRecord(c->ev_fork, s));
    HIP_TRY(c, hipStreamWaitEvent(aux, c->ev_fork, 0));
    const size_t k = ktimer_begin(c, pre + ".split", aux);
    HIP_TRY(c, launch_split_syrk(c->Dp, ap, aux));
    ktimer_end(c, k, aux);
  } else if (ap.n_work > 0) {
    const size_t k = ktimer_begin(c, pre + ".split", s);
    HIP_TRY(c, launch_split_syrk(c->Dp, ap, s));
    ktimer_end(c, k, s);
  }
  rc = prof_counters(c, c->d_prof, 16, &ap.prof);
  if (rc) return rc;
  const size_t k = ktimer_begin(c, pre + ".dspace", s);
  if (side_split) {
    SolveArgs af = ap;  // queue positions [0, n_split): the split entities
    af.n_rows = ap.n_split;
    HIP_TRY(c, launch_solve(c->Dp, af, aux));
    HIP_TRY(c, hipEventRecord(c->ev_join, aux));
    SolveArgs ar = ap;  // positions [n_split, n_rows)
    ar.order = ap.order + ap.n_split;
    ar.n_rows = ap.n_rows - ap.n_split;
    ar.split = nullptr;
    ar.n_split = 0;
    ar.work = nullptr;
    ar.n_work = 0;
    HIP_TRY(c, launch_solve(c->Dp, ar, s));
    HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join, 0));
  } else {
    HIP_TRY(c, launch_solve(c->Dp, ap, s));
  }
  ktimer_end(c, k, s);
  {  // the split entities' SYRK is the split kernel's work, their solve this one's
    const double d = c->dim;
    const HeffSums sp = heff_sums(c, side, vq, 0, ap.n_split);
    const HeffSums rest = heff_sums(c, side, vq, ap.n_split, ap.n_rows);
    const int64_t ne = sp.nz + rest.nz;
    add_work(c, pre + ".dspace",
             d * (d + 1.0) * rest.h1 + (double)ne * dspace_solve_flops(d),
             (d * 4.0 + 4.0) * rest.h1 + (double)ne * (8.0 + d * 4.0), ne);
    if (ap.n_work > 0)
      add_work(c, pre + ".split", d * (d + 1.0) * sp.h1, (d * 4.0 + 4.0) * sp.h1, sp.nz);
  }
  if (ap.prof) {  // diagnostics: mean cycles per entity and phase
    unsigned long long hp[16];
    HIP_TRY(c, hipStreamSynchronize(s));
    rc = prof_readback(c, c->d_prof, 16, hp);
    if (rc) return rc;
    const double n = (double)std::max<unsigned long long>(hp[4], 1);
    fprintf(stderr, "[dspace-prof] %s n %llu mean h %.0f cycles/entity: setup %.0f syrk %.0f "
            "epilogue %.0f (rhs %.0f tiles %.0f) chol %.0f | chain %.0f workers %.0f factored %.0f\n",
            pre.c_str(), hp[4], hp[8] / n, hp[0] / n, hp[1] / n, (hp[2] + hp[9] + hp[10]) / n,
            hp[9] / n, hp[10] / n, hp[3] / n, hp[5] / n, hp[6] / n, hp[7] / n);
    fprintf(stderr, "[dspace-prof] %s chain: waits %.0f trsm %.0f update %.0f factor %.0f | "
            "worker waits %.0f\n",
            pre.c_str(), hp[11] / n, hp[12] / n, hp[13] / n, hp[14] / n, hp[15] / n);
  }
  return FRECSYS_OK;
}

int launch_dspace(frecsys_ctx* c, int side, const SolveArgs& ap, hipStream_t s,
                  const std::string& pre, bool can_split, hipStream_t aux = nullptr) {
  return wide_dim(c->Dp) ? launch_dspace_wide(c, side, ap, s, pre, can_split)
                         : launch_dspace_tiled(c, side, ap, s, pre, can_split, aux);
}

// The argument checks frecsys_solve_side and frecsys_solve_side_cg share
// (pre: the call's message prefix; frecsys_pp_step has texts of its own).
int check_solve_args(frecsys_ctx* c, const std::string& pre, int side,
                     const frecsys_solve_params* p) {
  if (!c->rp[side]) return fail(c, FRECSYS_ERR_INVALID, pre + "no CSR loaded for side");
  const int kind = p->kind;
  if (kind < FRECSYS_KIND_IALS || kind > FRECSYS_KIND_CVAR_GRAD_V)
    return fail(c, FRECSYS_ERR_INVALID, pre + "bad kind");
  if (is_vkind(kind) && (!p->entity_reg || !p->other_weight))
    return fail(c, FRECSYS_ERR_INVALID, pre + "V kinds need entity_reg and other_weight");
  if (is_grad(kind) && side == 2)
    return fail(c, FRECSYS_ERR_INVALID, pre + "CVaR step on EVAL side");
  if (p->from_snapshot && !c->snap[side == 1 ? 0 : 1])
    return fail(c, FRECSYS_ERR_INVALID, pre + "from_snapshot without a snapshot");
  return FRECSYS_OK;
}

// What every solve entry point does before its launches: the device, the
// early basis builds of `eager_mask` joined, the per-entity vectors the kind
// reads uploaded, the failure word reset.
int begin_solve(frecsys_ctx* c, int side, const frecsys_solve_params* p, int eager_mask) {
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = join_eager(c, eager_mask, c->stream);
  if (rc) return rc;
  const int other = side == 1 ? 0 : 1;
  if (is_ukind(p->kind) && p->entity_weight) {
    rc = upload(c, c->d_entity_weight, p->entity_weight, (size_t)c->n[side]);
    if (rc) return rc;
  }
  if (is_vkind(p->kind)) {
    rc = upload(c, c->d_entity_reg, p->entity_reg, (size_t)c->n[side]);
    if (rc) return rc;
    rc = upload(c, c->d_other_weight, p->other_weight, (size_t)c->n[other]);
    if (rc) return rc;
  }
  // ~0ull by a device-side fill: an H2D copy from host memory at this point
  // was observed starting only after the early basis build queued on another
  // stream had finished, holding back the fork of the d-space solve
  HIP_TRY(c, hipMemsetAsync(c->d_fail, 0xFF, sizeof(unsigned long long), c->stream));
  return FRECSYS_OK;
}

// ... and after them: the failure word read back into *f (~0ull: none), the
// solved rows all-gathered (gather: the call has not exchanged them itself),
// the stream synchronised and the kernel timers resolved.
int end_solve(frecsys_ctx* c, int side, bool gather, unsigned long long* f) {
  HIP_TRY(c, hipMemcpyAsync(f, c->d_fail, sizeof(*f), hipMemcpyDeviceToHost, c->stream));
  if (gather && side < 2 && (c->world > 1 || c->comm)) {
    ScopedTimer t(c, "allgather");
    int rc = allgather_rows(c, c->emb[side], side, c->Dp);
    if (rc) return rc;
    t.stop();
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  flush_ktimers(c);
  return FRECSYS_OK;
}

// The d-space kernels' arguments for the rank's whole shard of `side` (the
// uploads of begin_solve and the queue of build_order are in place).
SolveArgs solve_args(frecsys_ctx* c, int side, const frecsys_solve_params* p) {
  const int other = side == 1 ? 0 : 1;
  int64_t lo, hi;
  shard(c, side, &lo, &hi);
  SolveArgs a{};
  a.kind = p->kind;
  a.order = c->d_order[side];
  a.counter = c->d_counter;
  a.quirk = c->quirks;
  a.row_ptr = c->rp[side];
  a.col = c->col[side];
  a.row_lo = lo;
  a.n_rows = hi - lo;
  a.X = p->from_snapshot ? c->snap[other] : c->emb[other];
  a.n_other = c->n[other];
  a.G = c->gram[other];
  a.E = c->emb[side];
  a.out = c->emb[side];
  a.reg = p->reg;
  a.reg_exp = p->reg_exp;
  a.w = p->unobserved_weight;
  a.alpha = p->alpha;
  a.eta = p->stepsize;
  a.lambda_is_reg = p->lambda_is_reg;
  a.entity_weight = (is_ukind(p->kind) && p->entity_weight) ? c->d_entity_weight.dev.get() : nullptr;
  a.entity_reg = is_vkind(p->kind) ? c->d_entity_reg.dev.get() : nullptr;
  a.other_weight = is_vkind(p->kind) ? c->d_other_weight.dev.get() : nullptr;
  a.fail = c->d_fail;
  a.debug_skip = c->debug_skip;
  a.chol_sched = c->chol_sched;
  return a;
}

// The history-space form needs M = mu*G + lam*I SPD for every entity:
// lam > 0 and mu >= 0 (G is PSD).  Otherwise (and when it reports a
// non-positive pivot) the call runs the d-space solve for everyone.
bool hspace_allowed(const frecsys_ctx* c, int side, const frecsys_solve_params* p) {
  const int other = side == 1 ? 0 : 1;
  bool m_spd = p->reg > 0.0f && p->unobserved_weight >= 0.0f;
  if (m_spd && is_ukind(p->kind) && p->entity_weight)
    for (int64_t i = 0; i < c->n[side] && m_spd; ++i) m_spd = p->entity_weight[i] >= 0.0f;
  if (m_spd && is_vkind(p->kind) && !p->lambda_is_reg) {
    const float base = p->alpha * p->unobserved_weight * (float)c->n[other];
    for (int64_t i = 0; i < c->n[side] && m_spd; ++i) m_spd = p->entity_reg[i] + base > 0.0f;
  }
  return m_spd;
}

// Queue split: the queue is sorted by decreasing history, and h_eff (the
// rows the assembly reads, tail-quirk rows included) is monotone in h, so
// the d-space entities are a prefix [0, n_dspace), then the history-space
// buckets (32*(t-1) < h_eff <= 32*t, t = 8..1) up to n_nonempty, then the
// empty histories.  Without history space (dual false) both are n_rows.
struct SidePlan {
  bool dual = false;
  int64_t n_dspace = 0, n_nonempty = 0;
  // one M = mu*G + lam*I for every entity (iALS with l2_reg_exp = 0, or
  // lambda = reg: ials.h:310-315): the Cholesky basis (bmode 1), no
  // tridiagonal reduction, no per-entity LDL -- at every Dp the history space
  // runs at (64..256, 512, 1024: chol_basis_kernel<T>, launch_chol_basis)
  int bmode = 0;
  float bmu = 0.f, blam = 0.f;
  std::string pre;  // the timer and work keys' prefix: solve_user / _item / _eval
};
SidePlan plan_side(const frecsys_ctx* c, int side, const frecsys_solve_params* p, int64_t n_rows,
                   bool force_dspace) {
  const bool vq = is_vkind(p->kind);
  SidePlan pl;
  pl.pre = kSolveNames[side];
  pl.dual = c->dual_on && !force_dspace && hspace_allowed(c, side, p) && !is_grad(p->kind) &&
            c->Dp >= 64 && c->dual_max_h_side[side] > 0 &&
            (int64_t)c->order_h[side].size() == c->order_n[side];
  pl.n_dspace = pl.dual ? first_le(c, side, vq, c->dual_max_h_side[side]) : n_rows;
  pl.n_nonempty = pl.dual ? first_le(c, side, vq, 0) : n_rows;
  if (c->chol_basis_on && p->kind == FRECSYS_KIND_IALS &&
      (p->lambda_is_reg || p->reg_exp == 0.0f)) {
    pl.bmode = 1;
    pl.bmu = p->unobserved_weight;
    pl.blam = p->reg;
  }
  return pl;
}

// The history-space kernels' arguments, from the d-space ones.
DualArgs dual_args(const frecsys_ctx* c, int side, const SolveArgs& a, const SidePlan& pl) {
  const int other = side == 1 ? 0 : 1;
  DualArgs d{};
  d.kind = a.kind;
  d.quirk = c->quirks;
  d.Dp = c->Dp;
  d.col = a.col;
  d.Xrot = c->xrot[other];
  d.tdiag = c->tri[other];
  d.toff = c->tri[other] + c->Dp;
  d.unit_m = pl.bmode;
  d.basis_status = c->tri[other];
  d.n_other = a.n_other;
  d.reg = a.reg;
  d.reg_exp = a.reg_exp;
  d.w = a.w;
  d.alpha = a.alpha;
  d.lambda_is_reg = a.lambda_is_reg;
  d.entity_weight = a.entity_weight;
  d.entity_reg = a.entity_reg;
  d.other_weight = a.other_weight;
  d.fail = a.fail;
  d.debug_skip = a.debug_skip;
  d.chol_sched = a.chol_sched;
  return d;
}

// The wide bucket, 256 < h_eff <= 512: queue positions [lo, hi) in batches
// of its workspace, on stream.
int launch_hspace_wide_bucket(frecsys_ctx* c, const SolveArgs& a, const SidePlan& pl, DualArgs d,
                              int64_t lo, int64_t hi) {
  const size_t per = dual_wide_zs_bytes(c->Dp) + sizeof(float) * (dual_wide_slot_floats() + 512);
  const size_t held = c->dw_zs.cap() + sizeof(float) * (c->dw_slots.cap() + c->dw_z.cap());
  int64_t nbat =
      std::max<int64_t>(1, std::min<int64_t>(hi - lo, (int64_t)(ws_budget(c, held) / per)));
  if (hi <= lo) return FRECSYS_OK;
  int rc = ensure_batch(c, c->dw_zs, dual_wide_zs_bytes(c->Dp), &nbat);
  if (rc) return rc;
  rc = ensure_batch(c, c->dw_slots, dual_wide_slot_floats(), &nbat);
  if (rc) return rc;
  rc = ensure_batch(c, c->dw_z, (size_t)512, &nbat);
  if (rc) return rc;
  d.prof = nullptr;
  for (int64_t b0 = lo; b0 < hi; b0 += nbat) {
    d.order = a.order + b0;
    d.n_rows = std::min(nbat, hi - b0);
    d.pos0 = b0 - pl.n_dspace;
    HIP_TRY(c, launch_dual_wide(d, c->dw_zs, c->dw_slots, c->dw_z, a.fail, c->stream));
  }
  return FRECSYS_OK;
}

// The history-space solve of queue positions [n_dspace, n_nonempty) in the
// basis prepare_basis left: the LDL table, the buckets, the sweep, and the
// rotation of the solved rows back into a.out.
int launch_hspace(frecsys_ctx* c, int side, const SolveArgs& a, const SidePlan& pl) {
  const int other = side == 1 ? 0 : 1;
  const bool vq = is_vkind(a.kind);
  const int64_t n_dspace = pl.n_dspace, n_nonempty = pl.n_nonempty;
  DualArgs d = dual_args(c, side, a, pl);
  unsigned long long* prof = nullptr;
  int rc = prof_counters(c, c->dual_prof, 16 * 9, &prof);
  if (rc) return rc;
  const int64_t n_hs = n_nonempty - n_dspace;
  const size_t n_blk = (size_t)((n_hs + 63) / 64) * 64;  // position-blocked buffers
  rc = ensure(c, c->dual_table, n_blk * 3 * c->Dp);
  if (rc) return rc;
  rc = ensure(c, c->out_rot[side], n_blk * c->Dp);
  if (rc) return rc;
  d.out_rot = c->out_rot[side];
  size_t k = ktimer_begin(c, pl.pre + ".hspace", c->stream);
  d.order = a.order + n_dspace;
  d.n_rows = n_hs;
  d.table = c->dual_table;
  d.pos0 = 0;
  HIP_TRY(c, launch_dual_ldl(d, c->stream));
  // buckets in two lanes (the long ones on stream, the short ones on
  // stream3) so one bucket's tail and resource shape overlap another's
  const bool two_lanes = !c->dual_serial;
  if (two_lanes) {
    HIP_TRY(c, hipEventRecord(c->ev_fork3, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream3, c->ev_fork3, 0));
  }
  int64_t lo = n_dspace;
  if (c->dual_max_h_side[side] > 32 * kDualMaxTiles && lo < n_nonempty) {
    const int64_t hi = std::min(n_nonempty, first_le(c, side, vq, 32 * kDualMaxTiles));
    rc = launch_hspace_wide_bucket(c, a, pl, d, lo, hi);
    if (rc) return rc;
    lo = std::max(lo, hi);
  }
  for (int tiles = kDualMaxTiles; tiles >= 1 && lo < n_nonempty; --tiles) {
    const int64_t hi = std::min(n_nonempty, first_le(c, side, vq, 32 * (tiles - 1)));
    if (hi > lo) {
      d.order = a.order + lo;
      d.n_rows = hi - lo;
      d.pos0 = lo - n_dspace;
      d.prof = prof ? prof + 16 * tiles : nullptr;
      hipStream_t ls = (two_lanes && tiles <= 4) ? c->stream3 : c->stream;
      HIP_TRY(c, launch_dual(tiles, d, ls));
    }
    lo = std::max(lo, hi);
  }
  if (two_lanes) {
    HIP_TRY(c, hipEventRecord(c->ev_join3, c->stream3));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join3, 0));
  }
  d.order = a.order + n_dspace;
  d.n_rows = n_hs;
  d.pos0 = 0;
  if (!pl.bmode) HIP_TRY(c, launch_dual_sweep(d, c->stream));  // unit table: identity
  ktimer_end(c, k, c->stream);
  {  // h x h system per entity: S = I + Z D^-1 Z^T (h^2 d), its LLT (h^3 / 3),
     // the recurrence and Y^T z (4 h d); rows read twice, the LDL row
    const double dd = c->dim;
    const HeffSums hsum = heff_sums(c, side, vq, n_dspace, n_nonempty);
    const double ne = (double)n_hs;
    add_work(c, pl.pre + ".hspace", hsum.h2 * dd + hsum.h3 / 3.0 + 4.0 * hsum.h1 * dd,
             (2.0 * dd * 4.0 + 4.0) * hsum.h1 + ne * (8.0 + 3.0 * dd * 4.0 + dd * 4.0), n_hs);
  }
  k = ktimer_begin(c, pl.pre + ".rotate", c->stream);
  HIP_TRY(c, launch_rotate(c->out_rot[side], a.order + n_dspace, 0, n_hs, c->qsplit[other][1],
                           a.out, c->Dp, c->stream, 1));
  ktimer_end(c, k, c->stream);
  return FRECSYS_OK;
}

// The mixed path: the d-space solve of the long histories on stream2,
// concurrently with the basis change + history-space solve of the rest on
// stream.  The basis (one-workgroup tridiagonalisation first) is queued
// before the d-space kernels so its workgroup is not left waiting for a CU
// behind them; stream2 waits only for what preceded the fork.
int launch_mixed(frecsys_ctx* c, int side, const SolveArgs& a, const SidePlan& pl) {
  const int other = side == 1 ? 0 : 1;
  hipStream_t s2 = c->dual_serial ? c->stream : c->stream2;
  if (pl.n_dspace > 0) HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
  c->want_mode[other] = pl.bmode;  // what an early build of the next Gramian prepares
  c->want_mu[other] = pl.bmu;
  c->want_lam[other] = pl.blam;
  const QueueRec* hrows = nullptr;
  int64_t nhrows = 0;
  uint64_t hsub = 0;
  int rc = hspace_rows(c, side, other, pl.n_dspace, pl.n_nonempty, &hrows, &nhrows, &hsub);
  if (rc) return rc;
  const size_t k = ktimer_begin(c, pl.pre + ".basis", c->stream);
  rc = prepare_basis(c, other, a.X, c->stream, pl.bmode, pl.bmu, pl.blam, hrows, nhrows, hsub);
  if (rc) return rc;
  ktimer_end(c, k, c->stream);
  if (pl.n_dspace > 0) {
    HIP_TRY(c, hipStreamWaitEvent(s2, c->ev_fork, 0));
    SolveArgs ap = a;
    ap.n_rows = pl.n_dspace;
    rc = launch_dspace(c, side, ap, s2, pl.pre, true);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_join, s2));
  }
  rc = launch_hspace(c, side, a, pl);  // allocates: after the d-space launch, a hipMalloc can block
  if (rc) return rc;
  if (pl.n_dspace > 0) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
  return FRECSYS_OK;
}

// FRECSYS_DUAL_PROF: mean cycles per entity and phase of the history-space
// workgroup kernel, per bucket.
int print_dual_prof(frecsys_ctx* c, int side) {
  unsigned long long hp[16 * 9];
  int rc = prof_readback(c, c->dual_prof, 16 * 9, hp);
  if (rc) return rc;
  for (int t = 1; t <= 8; ++t) {
    const unsigned long long n = hp[16 * t + 4];
    if (!n) continue;
    fprintf(stderr, "[dual-prof] side %d tiles %d n %llu cycles/entity: setup %.0f slabs %.0f chol %.0f "
            "yz %.0f | chain %.0f workers %.0f factored %.0f\n", side, t, n,
            (double)hp[16 * t] / n, (double)hp[16 * t + 1] / n, (double)hp[16 * t + 2] / n,
            (double)hp[16 * t + 3] / n, (double)hp[16 * t + 5] / n, (double)hp[16 * t + 6] / n,
            (double)hp[16 * t + 7] / n);
    // chol_solve_df's own counters (the workgroup buckets; the wave-per-entity
    // kernel of TH <= 2 has no chain)
    if (hp[16 * t + 14])
      fprintf(stderr, "[dual-prof] side %d tiles %d chain: waits %.0f trsm %.0f update %.0f factor %.0f "
              "| worker waits %.0f\n", side, t, (double)hp[16 * t + 11] / n,
              (double)hp[16 * t + 12] / n, (double)hp[16 * t + 13] / n, (double)hp[16 * t + 14] / n,
              (double)hp[16 * t + 15] / n);
  }
  return FRECSYS_OK;
}

int solve_side(frecsys_ctx* c, int32_t side, const frecsys_solve_params* p, bool force_dspace);

// What the failure word f (~0ull: none; else the smallest failing entity + 1,
// over all ranks with a communicator) means for the call.
int solve_verdict(frecsys_ctx* c, int side, const frecsys_solve_params* p, const SidePlan& pl,
                  unsigned long long f) {
  if (f == ~0ull) return FRECSYS_OK;
  // ablation builds only (FRECSYS_DEBUG_SKIP): the skipped phases leave
  // garbage matrices by design, so a failed pivot is expected and ignored
  // -- a timing run must reach the end of the epoch, not abort on NOT_SPD
  if (c->debug_skip) return FRECSYS_OK;
  if (pl.dual && ((side < 2 && c->comm) || pl.n_dspace < pl.n_nonempty)) {
    // a history-space pivot failed (or a poisoned basis after a tagged-poll
    // timeout): the verdict is the d-space solve's.  Counted (frecsys_counter
    // "hspace_reruns"): the whole side pays a d-space solve, a second full pass
    ++c->hspace_reruns;
    return solve_side(c, side, p, true);
  }
  c->err_entity = (int64_t)f - 1;
  return fail(c, FRECSYS_ERR_NOT_SPD,
              "LLT failed (matrix not SPD) for entity " + std::to_string(c->err_entity));
}

int solve_side(frecsys_ctx* c, int32_t side, const frecsys_solve_params* p, bool force_dspace) {
  if (!c || !valid_side(side) || !p) return fail(c, FRECSYS_ERR_INVALID, "solve: bad arguments");
  int rc = check_solve_args(c, "solve: ", side, p);
  if (rc) return rc;
  rc = begin_solve(c, side, p, side < 2 ? 1 << side : 0);  // a build still reading emb[side]
  if (rc) return rc;
  rc = build_order(c, side);
  if (rc) return rc;
  const SolveArgs a = solve_args(c, side, p);
  const SidePlan pl = plan_side(c, side, p, a.n_rows, force_dspace);
  c->dual_used[side] = pl.dual;
  if (side < 2) emb_written(c, side);
  {
    ScopedTimer t(c, kSolveNames[side]);
    if (pl.dual && pl.n_dspace < pl.n_nonempty) {
      rc = launch_mixed(c, side, a, pl);
    } else {
      // stream2 (the mixed path's d-space stream) is idle here: the slabs of
      // the long histories run on it beside the other entities' solve
      rc = launch_dspace(c, side, a, c->stream, pl.pre,
                         c->Dp >= 32 && (int64_t)c->order_h[side].size() == c->order_n[side],
                         c->dual_serial ? nullptr : c->stream2);
    }
    if (rc) return rc;
    t.stop();
  }
  if (side < 2 && c->comm) {
    // every rank takes the same retry / NOT_SPD decision (the smallest
    // failing entity over all ranks), so the collectives of a rerun stay
    // matched
    NCCL_TRY(c, ncclAllReduce(c->d_fail, c->d_fail, 1, ncclUint64, ncclMin, c->comm, c->stream));
  }
  unsigned long long f = ~0ull;
  rc = end_solve(c, side, true, &f);
  if (rc) return rc;
  if (dual_prof_on() && pl.dual && c->dual_prof) {
    rc = print_dual_prof(c, side);
    if (rc) return rc;
  }
  return solve_verdict(c, side, p, pl, f);
}

}  // namespace

extern "C" {

int frecsys_solve_side(frecsys_ctx* c, int32_t side, const frecsys_solve_params* p) {
  return solve_side(c, side, p, false);
}

// Conjugate-gradient form of frecsys_solve_side (cg.hip): the same sharding,
// queue, uploads and row all-gather; no factorisation, so no NOT_SPD.
int frecsys_solve_side_cg(frecsys_ctx* c, int32_t side, const frecsys_solve_params* p,
                          const frecsys_cg_params* cg) {
  if (!c || !valid_side(side) || !p || !cg)
    return fail(c, FRECSYS_ERR_INVALID, "solve_cg: bad arguments");
  if (cg->max_iterations < 0 || !(cg->tolerance >= 0.0f))
    return fail(c, FRECSYS_ERR_INVALID,
                "solve_cg: max_iterations and tolerance must be >= 0 (and not NaN)");
  const int kind = p->kind;
  if (kind == FRECSYS_KIND_CVAR_GRAD_U || kind == FRECSYS_KIND_CVAR_GRAD_V)
    return fail(c, FRECSYS_ERR_INVALID,
                "solve_cg: the CVaR gradient kinds have no conjugate-gradient form");
  if (c->dim > 256)
    return fail(c, FRECSYS_ERR_UNSUPPORTED,
                "solve_cg: the conjugate-gradient path is built for dim <= 256 (dim " +
                    std::to_string(c->dim) + ")");
  int rc = check_solve_args(c, "solve_cg: ", side, p);
  if (rc) return rc;
  const bool vkind = kind == FRECSYS_KIND_WEIGHTED_V;
  const bool ukind = kind == FRECSYS_KIND_WEIGHTED_U;
  const int other = side == 1 ? 0 : 1;
  rc = begin_solve(c, side, p, side < 2 ? 1 << side : 0);  // a build still reading emb[side]
  if (rc) return rc;
  rc = build_order(c, side);
  if (rc) return rc;
  const int64_t n = c->n[side];
  rc = ensure(c, c->d_cg_iters, (size_t)std::max<int64_t>(n, 1));
  if (rc) return rc;
  rc = ensure(c, c->d_cg_stats, (size_t)2);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(c->d_cg_iters, 0xFF, sizeof(int32_t) * std::max<int64_t>(n, 1),
                            c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_cg_stats, 0, sizeof(unsigned long long) * 2, c->stream));
  CgArgs a{};
  a.kind = kind;
  a.quirk = c->quirks;
  a.Dp = c->Dp;
  a.dim = c->dim;
  a.order = c->d_order[side];
  cg_plan_batches(c->h_order[side].data(), c->order_n[side], &c->cg_bstart);
  rc = ensure(c, c->d_cg_bstart, c->cg_bstart.size());
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_cg_bstart, c->cg_bstart.data(),
                            sizeof(int32_t) * c->cg_bstart.size(), hipMemcpyHostToDevice,
                            c->stream));
  a.bstart = c->d_cg_bstart;
  a.n_batches = (int64_t)c->cg_bstart.size() - 1;
  a.col = c->col[side];
  a.X = p->from_snapshot ? c->snap[other] : c->emb[other];
  a.n_other = c->n[other];
  a.G = c->gram[other];
  a.out = c->emb[side];
  a.reg = p->reg;
  a.reg_exp = p->reg_exp;
  a.w = p->unobserved_weight;
  a.alpha = p->alpha;
  a.lambda_is_reg = p->lambda_is_reg;
  a.entity_weight = (ukind && p->entity_weight) ? c->d_entity_weight.dev.get() : nullptr;
  a.entity_reg = vkind ? c->d_entity_reg.dev.get() : nullptr;
  a.other_weight = vkind ? c->d_other_weight.dev.get() : nullptr;
  a.max_iter = cg->max_iterations;
  a.tol = cg->tolerance;
  a.iters = c->d_cg_iters;
  a.stats = c->d_cg_stats;
  a.fail = c->d_fail;
  if (side < 2) emb_written(c, side);
  c->dual_used[side] = false;
  const std::string pre = kSolveNames[side];
  {
    ScopedTimer t(c, kSolveNames[side]);
    const size_t k = ktimer_begin(c, pre + ".cg", c->stream);
    HIP_TRY(c, launch_cg(a, c->stream));
    ktimer_end(c, k, c->stream);
    t.stop();
  }
  unsigned long long f = ~0ull, st[2] = {0, 0};
  std::vector<int32_t>& it = c->cg_iters[side];
  it.assign((size_t)n, -1);
  HIP_TRY(c, hipMemcpyAsync(st, c->d_cg_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  if (n)
    HIP_TRY(c, hipMemcpyAsync(it.data(), c->d_cg_iters, sizeof(int32_t) * n, hipMemcpyDeviceToHost,
                              c->stream));
  rc = end_solve(c, side, true, &f);
  if (rc) return rc;
  c->cg_iterations += (int64_t)st[0];
  c->cg_unconverged += (int64_t)st[1];
  {  // per entity and iteration: G p (2 d^2) + two passes of the history rows (4 h d)
    const double d = c->dim;
    const std::vector<QueueRec>& q = c->h_order[side];
    double fl = 0.0, by = 0.0;
    int64_t ne = 0;
    for (const QueueRec& r : q) {
      const int32_t i = it[(size_t)r.entity];
      if (i < 0) continue;
      ++ne;
      fl += (double)i * (2.0 * d * d + 4.0 * (double)r.h * d);
      by += (double)i * ((double)r.h * d * 4.0 + (double)r.h * 4.0);
    }
    add_work(c, pre + ".cg", fl, by, ne);
  }
  if (f != ~0ull) {
    c->err_entity = (int64_t)f - 1;
    return fail(c, FRECSYS_ERR_NAN,
                "solve_cg: non-finite result row for entity " + std::to_string(c->err_entity));
  }
  return FRECSYS_OK;
}

int frecsys_cg_iterations(frecsys_ctx* c, int32_t side, int32_t* host) {
  if (!c || !valid_side(side) || !host)
    return fail(c, FRECSYS_ERR_INVALID, "cg_iterations: bad arguments");
  const std::vector<int32_t>& it = c->cg_iters[side];
  for (int64_t i = 0; i < c->n[side]; ++i) host[i] = (size_t)i < it.size() ? it[(size_t)i] : -1;
  return FRECSYS_OK;
}

int frecsys_pp_set_rating_index(frecsys_ctx* c, int32_t side, const int32_t* rix) {
  if (!c || (side != 0 && side != 1) || !rix)
    return fail(c, FRECSYS_ERR_INVALID, "pp_set_rating_index: bad arguments");
  if (!c->rp[side]) return fail(c, FRECSYS_ERR_INVALID, "pp_set_rating_index: no CSR");
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t nnz = c->nnz[side];
  for (int64_t k = 0; k < nnz; ++k)
    if (rix[k] < 0 || rix[k] >= nnz)
      return fail(c, FRECSYS_ERR_INVALID, "pp_set_rating_index: index out of range");
  HIP_TRY(c, renew(c->d_rix[side], (size_t)nnz));
  if (nnz)
    HIP_TRY(c, hipMemcpy(c->d_rix[side], rix, sizeof(int32_t) * nnz, hipMemcpyHostToDevice));
  return ensure(c, c->d_pred[0], (size_t)std::max<int64_t>(nnz, 1));
}

namespace {
PPArgs pp_args(frecsys_ctx* c, int side) {
  const int other = side == 1 ? 0 : 1;
  PPArgs a{};
  a.col = c->col[side];
  a.rix = side == 2 ? nullptr : c->d_rix[side];
  a.pred = c->d_pred[side == 2 ? 1 : 0];
  a.X = c->emb[other];
  a.G = c->gram[other];
  a.E = c->emb[side];
  a.Dp = c->Dp;
  a.n_other = c->n[other];
  a.fail = c->d_fail;
  return a;
}
}  // namespace

int frecsys_pp_predict(frecsys_ctx* c, int32_t side) {
  if (!c || (side != 0 && side != 2)) return fail(c, FRECSYS_ERR_INVALID, "pp_predict: bad side");
  if (!c->rp[side]) return fail(c, FRECSYS_ERR_INVALID, "pp_predict: no CSR");
  if (side == 0 && !c->d_rix[0])
    return fail(c, FRECSYS_ERR_INVALID, "pp_predict: no rating index (pp_set_rating_index)");
  if (c->pp_old_side != -1)  // the other ranks' updates of the last block are not in yet
    return fail(c, FRECSYS_ERR_INVALID, "pp_predict: pp_sync pending for the last sharded block step");
  HIP_TRY(c, hipSetDevice(c->device));
  if (side == 2) {
    int rc = ensure(c, c->d_pred[1], (size_t)std::max<int64_t>(c->nnz[2], 1));
    if (rc) return rc;
  }
  PPArgs a = pp_args(c, side);
  HIP_TRY(c, launch_pp_predict(a, c->rp[side], c->n[side], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_pp_step(frecsys_ctx* c, int32_t side, int32_t start, int32_t end,
                    const frecsys_solve_params* p, double* residual) {
  if (!c || !valid_side(side) || !p) return fail(c, FRECSYS_ERR_INVALID, "pp_step: bad arguments");
  if (start < 0 || end > c->dim || end - start < 1 || end - start > 128)
    return fail(c, FRECSYS_ERR_INVALID, "pp_step: block must satisfy 0 <= start < end <= dim, "
                                        "end - start <= 128");
  if (!c->rp[side]) return fail(c, FRECSYS_ERR_INVALID, "pp_step: no CSR");
  if (side != 2 && !c->d_rix[side])
    return fail(c, FRECSYS_ERR_INVALID, "pp_step: no rating index (pp_set_rating_index)");
  if (!c->d_pred[side == 2 ? 1 : 0])
    return fail(c, FRECSYS_ERR_INVALID, "pp_step: no prediction vector (pp_predict)");
  const int kind = p->kind;
  if (kind != FRECSYS_KIND_IALS && kind != FRECSYS_KIND_WEIGHTED_U &&
      kind != FRECSYS_KIND_WEIGHTED_V)
    return fail(c, FRECSYS_ERR_INVALID, "pp_step: kind must be IALS, WEIGHTED_U or WEIGHTED_V");
  if (kind == FRECSYS_KIND_WEIGHTED_V && (!p->entity_reg || !p->other_weight))
    return fail(c, FRECSYS_ERR_INVALID, "pp_step: WEIGHTED_V needs entity_reg and other_weight");
  // external-exchange mode: a second step before frecsys_pp_sync would
  // overwrite the snapshot the other ranks' prediction updates are replayed
  // from, and this rank's predictions would drift from theirs
  if (c->pp_old_side != -1)
    return fail(c, FRECSYS_ERR_INVALID, "pp_step: pp_sync pending for the last sharded block step");
  int rc = begin_solve(c, side, p, 3);
  if (rc) return rc;
  if (side < 2) emb_written(c, side);
  // world > 1 (USER / ITEM): this rank's shard of the rows -- the per-row
  // block steps are independent given the predictions, which every rank then
  // brings up to date for the other ranks' rows (pp_refresh_kernel, bitwise
  // the owner's update); EVAL rows are not sharded
  const bool sharded = side < 2 && c->world > 1;
  const bool xchg = sharded && in_call_exchange(c);  // RCCL or the caller's transport
  int64_t lo, hi;
  shard(c, side, &lo, &hi);
  const int bw = end - start;
  if (sharded) {  // the block columns before the step: the refresh replays Delta from them
    rc = ensure(c, c->d_pp_old, (size_t)std::max<int64_t>(c->n[side], 1) * bw);
    if (rc) return rc;
    if (c->n[side])
      HIP_TRY(c, hipMemcpy2DAsync(c->d_pp_old, sizeof(float) * bw, c->emb[side] + start,
                                  sizeof(float) * c->Dp, sizeof(float) * bw, c->n[side],
                                  hipMemcpyDeviceToDevice, c->stream));
  }
  // the side's queue: the shard's rows by decreasing h (stable), the order the
  // residuals are summed in
  rc = build_order(c, side);
  if (rc) return rc;
  const std::vector<QueueRec>& recs = c->h_order[side];
  rc = ensure(c, c->d_resid, std::max<size_t>(recs.size(), 1));
  if (rc) return rc;
  PPArgs a = pp_args(c, side);
  a.order = c->d_order[side];
  a.n_rows = (int64_t)recs.size();
  a.start = start;
  a.bw = end - start;
  a.kind = kind;
  a.reg = p->reg;
  a.reg_exp = p->reg_exp;
  a.w = p->unobserved_weight;
  a.alpha = p->alpha;
  a.entity_weight =
      (kind == FRECSYS_KIND_WEIGHTED_U && p->entity_weight) ? c->d_entity_weight.dev.get() : nullptr;
  a.entity_reg = kind == FRECSYS_KIND_WEIGHTED_V ? c->d_entity_reg.dev.get() : nullptr;
  a.other_weight = kind == FRECSYS_KIND_WEIGHTED_V ? c->d_other_weight.dev.get() : nullptr;
  a.resid = c->d_resid;
  const unsigned long long none = ~0ull;
  {
    ScopedTimer t(c, "pp_step");
    HIP_TRY(c, launch_pp_step(a, c->stream));
    if (sharded && !xchg) {  // the caller exchanges the rows, then frecsys_pp_sync
      c->pp_old_side = side;
      c->pp_old_start = start;
      c->pp_old_bw = bw;
    }
    if (xchg) {
      // the rows of every rank, then the other ranks' prediction updates
      rc = xchg_rows(c, c->emb[side], side, c->Dp);
      if (rc) return rc;
      HIP_TRY(c, launch_pp_refresh(a, c->rp[side], c->d_pp_old, c->n[side], lo, hi, c->stream));
    }
    t.stop();
  }
  if (xchg) {  // every rank takes the same NOT_SPD verdict
    rc = xchg_min_u64(c, c->d_fail);
    if (rc) return rc;
  }
  std::vector<float> res(recs.size());
  unsigned long long f = none;
  if ((residual || xchg) && !recs.empty())
    HIP_TRY(c, hipMemcpyAsync(res.data(), c->d_resid, sizeof(float) * recs.size(),
                              hipMemcpyDeviceToHost, c->stream));
  rc = end_solve(c, side, false, &f);  // the rows were exchanged under the step's timer
  if (rc) return rc;
  if (f != none) {
    c->err_entity = (int64_t)(f - 1);
    return fail(c, FRECSYS_ERR_NOT_SPD, "pp_step: block matrix not SPD");
  }
  double s = 0.0;
  if (xchg) {
    // every rank's per-row residuals (all-gathered as a one-column table,
    // whether or not this rank asked for the sum: the ranks' exchanges stay
    // in step), summed in the single-rank queue order -- every row of the
    // side by decreasing h: the world-1 sum bit for bit
    const int64_t n = c->n[side];
    const std::vector<int64_t>& rp = c->host_rp[side];
    std::vector<int32_t>& all = c->pp_order_all[side];
    if ((int64_t)all.size() != n) {
      all.resize((size_t)n);
      for (int64_t i = 0; i < n; ++i) all[i] = (int32_t)i;
      std::stable_sort(all.begin(), all.end(), [&](int32_t x, int32_t y) {
        return rp[x + 1] - rp[x] > rp[y + 1] - rp[y];
      });
    }
    std::vector<float> ent((size_t)std::max<int64_t>(n, 1), 0.0f);
    for (size_t i = 0; i < recs.size(); ++i) ent[recs[i].entity] = res[i];
    rc = ensure(c, c->d_resid_e, (size_t)std::max<int64_t>(n, 1));
    if (rc) return rc;
    if (n) HIP_TRY(c, hipMemcpyAsync(c->d_resid_e, ent.data(), sizeof(float) * n,
                                     hipMemcpyHostToDevice, c->stream));
    rc = xchg_rows(c, c->d_resid_e, side, 1);
    if (rc) return rc;
    if (n) HIP_TRY(c, hipMemcpyAsync(ent.data(), c->d_resid_e, sizeof(float) * n,
                                     hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int32_t e : all) s += (double)ent[e];
  } else {
    for (float v : res) s += (double)v;  // zero rows (empty histories) stay 0
  }
  if (residual) *residual = s;
  return FRECSYS_OK;
}

int frecsys_pp_get_predictions(frecsys_ctx* c, int32_t side, float* host) {
  if (!c || (side != 0 && side != 2) || !host)
    return fail(c, FRECSYS_ERR_INVALID, "pp_get_predictions: bad arguments");
  const float* p = c->d_pred[side == 2 ? 1 : 0];
  if (!p) return fail(c, FRECSYS_ERR_INVALID, "pp_get_predictions: no prediction vector");
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t nnz = c->nnz[side];
  if (nnz)
    HIP_TRY(c, hipMemcpyAsync(host, p, sizeof(float) * nnz, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FRECSYS_OK;
}

int frecsys_pp_sync(frecsys_ctx* c, int32_t side) {
  if (!c || (side != 0 && side != 1)) return fail(c, FRECSYS_ERR_INVALID, "pp_sync: bad side");
  if (c->pp_old_side != side)
    return fail(c, FRECSYS_ERR_INVALID, "pp_sync: no sharded block step of this side pending");
  HIP_TRY(c, hipSetDevice(c->device));
  int64_t lo, hi;
  shard(c, side, &lo, &hi);
  PPArgs a = pp_args(c, side);
  a.start = c->pp_old_start;
  a.bw = c->pp_old_bw;
  HIP_TRY(c, launch_pp_refresh(a, c->rp[side], c->d_pp_old, c->n[side], lo, hi, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->pp_old_side = -1;
  return FRECSYS_OK;
}

}  // extern "C"
