// serve.hip -- host side of the ranking and evaluation calls of the C-ABI
// (include/frecsys_hip.h) that take a context and drive the device.  The
// context-free host calls are serve_host.hip's; serve.h holds what the two
// units share.  No kernels here: recommend.hip, similar.hip, rerank.hip,
// sampled.hip, metrics.hip, positions.hip, explain.hip, diversify.hip, dpp.hip,
// quality.hip and twostage.hip hold them (kernels.h).
//
// Workspace.  Every call carves the one byte buffer c->d_rec into 16-byte
// aligned typed regions (Carver): first the regions of a row batch (candidate
// slots or ids, bitmaps, the lists, the metric rows), then what the call needs
// once (eligibility words, candidate pointers, query row ids, ground truth,
// tables, cut-offs).  The budget (workspace_budget) bounds the batch regions
// only.
//
// Drivers.  A call runs its rows in batches, one timed launch group each, and
// synchronises after each batch's copy-back:
//   scan (scan_impl with one object behind the scan: recommend,
//     rank_metrics, recommend_diverse, recommend_dpp, rank_quality, and
//     recommend_two_stage with the bf16 scan in the fp32 scan's place; similar
//     and audience above its thin-query limit, with loops of their own):
//     budget / bytes per row, the scan's and what is behind it, in whole 64-row
//     blocks, with the item splits of scan_plan; a selection forms its Gramians
//     in sub-batches, within a budget of their own;
//   thin queries (audience): frecsys_audience_plan's splits and batch, per
//     query its lists per split, one reduce round's lists, bits and outputs;
//   pools (pools_impl: diversify, diversify_dpp): budget / bytes per row (the
//     pool, its Gramian, the selection), at least one row;
//   candidate lists (rank_candidates; cand_metrics_impl for
//     rank_candidates_metrics): rows in order while their fixed bytes and ids
//     fit the budget (cut_by_candidates); sampled lists (sampled_metrics): by
//     their fixed bytes within half the budget, then by ids within the other;
//   caller lists (lists_quality): budget / bytes per row (the list and the
//     result rows), at least one row;
//   pairs (score_pairs): budget / 16 B, at least 64;
//   positions (rank_positions): cut_by_candidates by the ground-truth entries;
//   explanations (explain): the same cut by the contributions, h floats per
//     (row, target) pair.
// Rows are independent, so the batch size never changes a result.
//
// Checks.  Each entry point keeps its own order of checks and its own point
// of return for zero rows; the checkers below are its pieces.
#include <climits>
#include <cstdlib>
#include <cstring>
#include <optional>

#include "serve.h"

namespace {

// The side (USER or `other`), k (nullptr: the call has none) and the flags.
int check_query(frecsys_ctx* c, const std::string& w, int32_t side, int32_t other,
                const int32_t* k, int32_t flags, int32_t known_flags) {
  if (side != FRECSYS_SIDE_USER && side != other)
    return fail(c, FRECSYS_ERR_INVALID,
                w + "side must be USER or " + (other == FRECSYS_SIDE_EVAL ? "EVAL" : "ITEM"));
  if (k && (*k < 1 || *k > 1024)) return fail(c, FRECSYS_ERR_INVALID, w + "k must be in [1, 1024]");
  if (flags & ~known_flags) return fail(c, FRECSYS_ERR_INVALID, w + "unknown flag");
  return FRECSYS_OK;
}

// The context's state and the query rows: a CSR to exclude from, both tables,
// row ids within the side (or no more rows than it has), and items to rank
// when the table searched is not the side's own.
int check_rows(frecsys_ctx* c, const std::string& w, int32_t side, int32_t table, bool exclude,
               const int64_t* rows, int64_t n) {
  if (exclude && !c->rp[side])
    return fail(c, FRECSYS_ERR_INVALID, w + "exclude flag on a side with no CSR loaded");
  if (!c->emb[side] || !c->emb[table])
    return fail(c, FRECSYS_ERR_INVALID, w + "side has no embeddings yet");
  const int64_t ns = c->n[side];
  if (rows) {
    for (int64_t i = 0; i < n; ++i)
      if (rows[i] < 0 || rows[i] >= ns)
        return fail(c, FRECSYS_ERR_INVALID,
                    w + "row id " + std::to_string(rows[i]) + " out of range");
  } else if (n > ns) {
    return fail(c, FRECSYS_ERR_INVALID, w + "more rows than the side has");
  }
  if (table != side && c->n[table] < 1)
    return fail(c, FRECSYS_ERR_INVALID, w + (table == FRECSYS_SIDE_USER ? "no users" : "no items"));
  return FRECSYS_OK;
}

// A candidate CSR over n rows with ids in [0, m).
int check_candidates(frecsys_ctx* c, const std::string& w, const int64_t* cand_ptr,
                     const int32_t* cand_items, int64_t n, int64_t m) {
  if (cand_ptr[0] != 0) return fail(c, FRECSYS_ERR_INVALID, w + "cand_ptr[0] must be 0");
  for (int64_t i = 0; i < n; ++i)
    if (cand_ptr[i + 1] < cand_ptr[i])
      return fail(c, FRECSYS_ERR_INVALID, w + "cand_ptr not monotone at row " + std::to_string(i));
  if (cand_ptr[n] > 0 && !cand_items) return fail(c, FRECSYS_ERR_INVALID, w + "null cand_items");
  for (int64_t p = 0; p < cand_ptr[n]; ++p)
    if (cand_items[p] < 0 || cand_items[p] >= m)
      return fail(c, FRECSYS_ERR_INVALID,
                  w + "candidate id " + std::to_string(cand_items[p]) + " out of range");
  return FRECSYS_OK;
}

// A cut-off list; *k = its largest, the length of the lists to rank.
int check_cutoffs(frecsys_ctx* c, const std::string& w, const int32_t* k_list, int32_t nk,
                  int32_t* k) {
  if (!k_list || nk < 1 || nk > kMetricMaxCutoffs)
    return fail(c, FRECSYS_ERR_INVALID,
                w + "k_list must hold 1 to " + std::to_string(kMetricMaxCutoffs) + " cut-offs");
  *k = 0;
  for (int32_t q = 0; q < nk; ++q) {
    if (k_list[q] < 1 || k_list[q] > kMetricMaxK)
      return fail(c, FRECSYS_ERR_INVALID, w + "cut-offs must be in [1, 1024]");
    *k = std::max(*k, k_list[q]);
  }
  return FRECSYS_OK;
}

// The carver of c->d_rec.  take<T>(count) hands out the next 16-byte aligned
// region.  A call states its layout once, in a function that run() calls
// twice: the first pass only sizes (the pointers it returns are offsets from
// zero, not to be used), then the buffer grows to the total, and the second
// pass returns the device pointers.
class Carver {
  uintptr_t base_ = 0;
  size_t used_ = 0;

 public:
  template <typename T>
  T* take(size_t count) {
    const size_t at = (used_ + 15) & ~(size_t)15;
    used_ = at + count * sizeof(T);
    return reinterpret_cast<T*>(base_ + at);
  }
  // A region some calls do without: no bytes and nullptr then.
  template <typename T>
  T* take_if(bool wanted, size_t count) {
    T* p = take<T>(wanted ? count : 0);
    return wanted ? p : nullptr;
  }
  template <typename Layout>
  static int run(frecsys_ctx* c, Layout layout) {
    Carver cv;
    layout(cv);
    const int rc = ensure(c, c->d_rec, cv.used_);
    if (rc) return rc;
    cv.base_ = reinterpret_cast<uintptr_t>((char*)c->d_rec);
    cv.used_ = 0;
    layout(cv);
    return FRECSYS_OK;
  }
};

template <typename T>
hipError_t to_device(frecsys_ctx* c, const T* dst, const T* src, size_t count) {
  return hipMemcpyAsync(const_cast<T*>(dst), src, sizeof(T) * count, hipMemcpyHostToDevice,
                        c->stream);
}
template <typename T>
hipError_t to_host(frecsys_ctx* c, T* dst, const T* src, size_t count) {
  return hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream);
}

// Eligibility bits of the m items: the mask and id < m.
std::vector<uint32_t> item_mask_words(int64_t m, const uint8_t* mask) {
  std::vector<uint32_t> maskw((size_t)recommend_words(m), 0u);
  for (int64_t j = 0; j < m; ++j)
    if (!mask || mask[j]) maskw[(size_t)(j >> 5)] |= 1u << (j & 31);
  return maskw;
}

// The scan of a table of m rows for n query rows: item splits -- about 2
// workgroups per CU over the call's 64-row blocks, within what the merge keeps
// in LDS, or what the splits knob says (read per call) -- and the rows of a
// batch: per row its candidates, counts and outputs, and per_row_extra bytes.
struct ScanPlan {
  int splits, cap;
  int64_t nb;
};
ScanPlan scan_plan(const frecsys_ctx* c, int k, int64_t m, int64_t n, size_t per_row_extra) {
  int dev_cus = 256;
  (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c->device);
  const int max_splits = recommend_max_splits(k, m);
  const int64_t row_blocks = (n + 63) / 64;
  int splits = (int)std::min<int64_t>(max_splits, (2 * (int64_t)dev_cus + row_blocks - 1) / row_blocks);
  if (const char* v = getenv("FRECSYS_RECOMMEND_SPLITS"))
    if (atoi(v) > 0) splits = std::min(max_splits, atoi(v));
  splits = std::max(1, splits);
  const int cap = recommend_cap(k);
  const size_t per_row =
      (size_t)splits * cap * 8 + (size_t)splits * 4 + (size_t)k * 8 + per_row_extra;
  int64_t nb = std::max<int64_t>(1, (int64_t)(workspace_budget() / per_row));
  if (nb < n && nb >= 64) nb &= ~(int64_t)63;  // whole 64-row blocks but in the last batch
  return {splits, cap, std::min(nb, n)};
}

// The scan's arguments but the batch, and its regions: per row of a batch the
// candidates, counts, history bits (when a CSR is excluded) and outputs, then
// the eligibility words and the query row ids.
RecommendArgs scan_args(const frecsys_ctx* c, int side, int table, int k, int splits,
                        bool exclude) {
  RecommendArgs a{};
  a.X = c->emb[side];
  a.Y = c->emb[table];
  a.m = c->n[table];
  a.Dp = c->Dp;
  a.k = k;
  a.splits = splits;
  a.row_ptr = exclude ? c->rp[side] : nullptr;
  a.col = exclude ? c->col[side] : nullptr;
  return a;
}
void carve_scan(Carver& cv, RecommendArgs& a, const ScanPlan& p, bool rows, int64_t n) {
  const size_t nb = (size_t)p.nb, W = (size_t)recommend_words(a.m);
  a.cand = cv.take<unsigned long long>(nb * p.splits * p.cap);
  a.counts = cv.take<int32_t>(nb * p.splits);
  a.bitmap = cv.take_if<uint32_t>(a.row_ptr != nullptr, nb * W);
  a.out_items = cv.take<int32_t>(nb * a.k);
  a.out_scores = cv.take<float>(nb * a.k);
  a.maskw = cv.take<uint32_t>(W);
  a.qrows = cv.take_if<int64_t>(rows, (size_t)n);
}

// Rows cut greedily in row order into batches whose bytes -- row_fixed per
// row and per_id (4: the id alone) per candidate id -- stay within the budget
// (at least one row each); the workspace is sized for the largest.
struct Cuts {
  std::vector<int64_t> cuts{0};
  int64_t max_rows = 0, max_ids = 0;
};
Cuts cut_by_candidates(const int64_t* ptr, int64_t n, size_t row_fixed, size_t budget,
                       size_t per_id = 4) {
  Cuts r;
  for (int64_t r0 = 0; r0 < n;) {
    size_t bytes = 0;
    int64_t r1 = r0;
    while (r1 < n) {
      const size_t add = row_fixed + (size_t)(ptr[r1 + 1] - ptr[r1]) * per_id;
      if (r1 > r0 && bytes + add > budget) break;
      bytes += add;
      ++r1;
    }
    r.max_rows = std::max(r.max_rows, r1 - r0);
    r.max_ids = std::max(r.max_ids, ptr[r1] - ptr[r0]);
    r.cuts.push_back(r1);
    r0 = r1;
  }
  return r;
}

// What the two candidate rankings share of RankCandArgs.
RankCandArgs cand_args(const frecsys_ctx* c, int side, int k, bool exclude) {
  RankCandArgs a{};
  a.X = c->emb[side];
  a.Y = c->emb[1];
  a.m = c->n[1];
  a.Dp = c->Dp;
  a.k = k;
  a.row_ptr = exclude ? c->rp[side] : nullptr;
  a.col = exclude ? c->col[side] : nullptr;
  return a;
}

// A batch's lists on their way to the host (the caller synchronises).
int copy_lists(frecsys_ctx* c, int32_t* items, float* scores, int k, int64_t r0, int64_t cnt,
               const int32_t* d_items, const float* d_scores) {
  HIP_TRY(c, to_host(c, items + r0 * k, d_items, (size_t)(cnt * k)));
  if (scores) HIP_TRY(c, to_host(c, scores + r0 * k, d_scores, (size_t)(cnt * k)));
  return FRECSYS_OK;
}

// What lies behind the scan of a ranking call (scan_impl).  Every step is
// virtual: a stage states its own with `override`, so a misnamed one fails to
// compile.
struct BehindScan {
  virtual size_t scan_bytes() const { return 0; }                // per row of a batch
  virtual void scan_carve(Carver&, int64_t) {}                   // regions: per row, then per call
  virtual int scan_upload(frecsys_ctx*) { return FRECSYS_OK; }   // per call, before the first batch
  virtual int scan_overlap(frecsys_ctx*) { return FRECSYS_OK; }  // host work during the first scan
  // a batch's lists and scores, where the scan left them
  virtual int run(frecsys_ctx* c, const int32_t* lists, const float* scores, int64_t r0,
                  int64_t cnt) = 0;
  virtual void book(frecsys_ctx*) const {}
  // after the last batch: what is left to fetch, and the work booked
  virtual int finish(frecsys_ctx* c) {
    book(c);
    return FRECSYS_OK;
  }
  virtual void no_rows(const frecsys_ctx*) const {}  // a call of zero rows passed its checks
};

// frecsys_recommend: the lists and (unless null) the scores go to the host.
struct ListsOut : BehindScan {
  int32_t* items;
  float* scores;
  int k;
  ListsOut(int32_t* i, float* s, int k_) : items(i), scores(s), k(k_) {}
  int run(frecsys_ctx* c, const int32_t* lists, const float* list_scores, int64_t r0,
          int64_t cnt) override {
    return copy_lists(c, items, scores, k, r0, cnt, lists, list_scores);
  }
};

// frecsys_recommend_two_stage behind its bf16 scan: the item table's image is
// built before the first batch (ts_convert_kernel, per call: the tables change
// with every solve), the scan leaves a batch's pools where `lists` / `scores`
// point, ts_select_kernel re-scores them there and the lists, the certificate
// bytes and (if asked for) the pools go to the host.  Per row of a batch: the
// list and its byte; per call: the stage's own copy of the query row ids.
struct TwoStageStage final : BehindScan {
  const int64_t* rows;
  const int64_t n;
  int32_t* items;
  float* scores;
  std::vector<uint8_t> cert;  // [n], on the host for the fallback; sized behind the checks
  int32_t* pool_items;
  float* pool_scores;
  TwoStageSelectArgs sa{};
  int64_t* d_rows = nullptr;

  TwoStageStage(const frecsys_ctx* c, int side, const int64_t* r, int64_t n_rows, int k, int pool,
                int32_t* i, float* s, int32_t* pi, float* ps)
      : rows(r), n(n_rows), items(i), scores(s), pool_items(pi), pool_scores(ps) {
    sa.X = c->emb[side];
    sa.Y = c->emb[1];
    sa.Dp = c->Dp;
    sa.k = k;
    sa.pool = pool;
  }
  size_t scan_bytes() const override { return (size_t)sa.k * 8 + 1; }
  void scan_carve(Carver& cv, int64_t nb) override {
    sa.out_items = cv.take<int32_t>((size_t)nb * sa.k);
    sa.out_scores = cv.take<float>((size_t)nb * sa.k);
    sa.certified = cv.take<uint8_t>((size_t)nb);
    d_rows = cv.take_if<int64_t>(rows != nullptr, (size_t)n);
  }
  // the image lies outside the per-row budget, in buffers of its own
  int scan_upload(frecsys_ctx* c) override {
    const int64_t m = c->n[1];
    cert.assign((size_t)n, 0);  // n is within the side's rows here
    int rc = ensure(c, c->d_ts_img, two_stage_image_bytes(m, c->Dp));
    if (!rc) rc = ensure(c, c->d_ts_norm, (size_t)m);
    if (!rc) rc = ensure(c, c->d_ts_stats, 2);
    if (rc) return rc;
    if (rows) HIP_TRY(c, to_device(c, d_rows, rows, (size_t)n));
    sa.qrows = d_rows;
    sa.stats = c->d_ts_stats;
    ScopedTimer t(c, "two_stage.convert");
    HIP_TRY(c, launch_two_stage_convert(c->emb[1], m, c->Dp, c->d_ts_img, c->d_ts_norm,
                                        c->d_ts_stats, c->stream));
    t.stop();
    return FRECSYS_OK;
  }
  int run(frecsys_ctx* c, const int32_t* lists, const float* list_scores, int64_t r0,
          int64_t cnt) override {
    sa.r0 = r0;
    sa.n = cnt;
    sa.pool_items = lists;
    sa.pool_scores = list_scores;
    ScopedTimer t(c, "two_stage.select");
    HIP_TRY(c, launch_two_stage_select(sa, c->stream));
    t.stop();
    HIP_TRY(c, to_host(c, cert.data() + r0, sa.certified, (size_t)cnt));
    if (pool_items) HIP_TRY(c, to_host(c, pool_items + r0 * sa.pool, lists, (size_t)cnt * sa.pool));
    if (pool_scores)
      HIP_TRY(c, to_host(c, pool_scores + r0 * sa.pool, list_scores, (size_t)cnt * sa.pool));
    return copy_lists(c, items, scores, sa.k, r0, cnt, sa.out_items, sa.out_scores);
  }
  // convert: a square-and-add per value; the table read, the image and the
  // norms written.  select: every slot booked as filled; flops at the logical
  // dim; one padded item row per slot, the pool read, the list written
  void book(frecsys_ctx* c) const override {
    const double m = (double)c->n[1], P = sa.pool;
    add_work(c, "two_stage.convert", 2.0 * m * c->dim,
             m * c->Dp * 4.0 + (double)two_stage_image_bytes(c->n[1], c->Dp) + m * 8.0, c->n[1]);
    add_work(c, "two_stage.select", 2.0 * (double)n * P * c->dim,
             (double)n * (P * (c->Dp * 4.0 + 8.0) + sa.k * 8.0 + 1.0), n);
  }
};

// What the metric calls add to a ranking call.
struct MetricsRequest {
  const int64_t* gt_ptr;
  const int32_t* gt_items;
  const int32_t* k_list;
  int32_t nk;
  float* recall;
  float* ndcg;
};

// The metrics behind a ranking of n rows into lists of k: the lists stay on
// the device, rank_metrics_kernel reads them there and 2 nk floats per row go
// to the host.  The order of its steps is the caller's: sort() before or
// during the first scan, the regions where the call's layout has them.
struct MetricsStage final : BehindScan {
  const MetricsRequest& mt;
  const int64_t n;
  const size_t nk;
  RankMetricsArgs ma{};
  std::vector<int64_t> sp;  // the ground truth as sets (sorted_ground_truth)
  std::vector<int32_t> sg;

  MetricsStage(const MetricsRequest& r, int64_t rows, int k) : mt(r), n(rows), nk((size_t)r.nk) {
    ma.k = k;
    ma.nk = r.nk;
  }
  void sort() { sorted_ground_truth(n, mt.gt_ptr, mt.gt_items, &sp, &sg); }
  // per call: the ground truth (room for gt_room ids), the tables, the cut-offs
  void carve_inputs(Carver& cv, size_t gt_room) {
    ma.gt_ptr = cv.take<int64_t>((size_t)n + 1);
    ma.gt = cv.take<int32_t>(gt_room);
    ma.gain = cv.take<double>(kMetricMaxK);
    ma.idcg = cv.take<double>(kMetricMaxK + 1);
    ma.k_list = cv.take<int32_t>(nk);
  }
  // per row of a batch: the two metric rows
  void carve_rows(Carver& cv, int64_t nb) {
    ma.recall = cv.take<float>((size_t)nb * nk);
    ma.ndcg = cv.take<float>((size_t)nb * nk);
  }
  int upload(frecsys_ctx* c) {
    const MetricTables& tab = metric_tables();
    HIP_TRY(c, to_device(c, ma.gt_ptr, sp.data(), sp.size()));
    HIP_TRY(c, to_device(c, ma.gt, sg.data(), sg.size()));
    HIP_TRY(c, to_device(c, ma.gain, tab.gain, (size_t)kMetricMaxK));
    HIP_TRY(c, to_device(c, ma.idcg, tab.idcg, (size_t)kMetricMaxK + 1));
    HIP_TRY(c, to_device(c, ma.k_list, mt.k_list, nk));
    return FRECSYS_OK;
  }
  // rows [r0, r0 + cnt) of the call, their lists at `lists`; the metric rows
  // are on their way to the host when it returns (the caller synchronises)
  int run(frecsys_ctx* c, const int32_t* lists, const float*, int64_t r0, int64_t cnt) override {
    ma.lists = lists;
    ma.r0 = r0;
    ma.n = cnt;
    ScopedTimer t(c, "rank_metrics");
    HIP_TRY(c, launch_rank_metrics(ma, c->stream));
    t.stop();
    HIP_TRY(c, to_host(c, mt.recall + r0 * nk, ma.recall, (size_t)cnt * nk));
    HIP_TRY(c, to_host(c, mt.ndcg + r0 * nk, ma.ndcg, (size_t)cnt * nk));
    return FRECSYS_OK;
  }
  // behind the scan: room for every id (repeats are dropped); the ground truth
  // is sorted while the first batch is scanned, and uploaded behind it
  size_t scan_bytes() const override { return nk * 8; }
  void scan_carve(Carver& cv, int64_t nb) override {
    carve_inputs(cv, (size_t)mt.gt_ptr[n]);
    carve_rows(cv, nb);
  }
  int scan_overlap(frecsys_ctx* c) override {
    sort();
    return upload(c);
  }
  // two double divisions per (row, cut-off); bytes: the lists and the ground
  // truth read, the metric rows written
  void book(frecsys_ctx* c) const override {
    add_work(c, "rank_metrics", 2.0 * (double)n * (double)nk,
             (double)n * ma.k * 4.0 + (double)sg.size() * 4.0 + ((double)n + 1.0) * 8.0 +
                 (double)n * (double)nk * 8.0,
             n);
  }
};

// What the MMR and DPP calls add to a ranking: the selection and where it goes
// (host; extra: the MMR values or gains, or nullptr; items null: it stays on
// the device for QualityStage).
struct PoolRequest {
  int32_t k, flags;
  int32_t* items;
  float* scores;
  float* extra;
};

// FRECSYS_DIVERSIFY_VARIANT (read per call; changes no result bit): "gram"
// forms the pool Gramians, "lazy" computes a Gramian row per step in the
// selection and needs no Gramian workspace; unset: kDiversifyLazyDefault.
constexpr bool kDiversifyLazyDefault = false;
bool diversify_lazy() {
  const char* v = getenv("FRECSYS_DIVERSIFY_VARIANT");
  if (v && !strcmp(v, "lazy")) return true;
  if (v && !strcmp(v, "gram")) return false;
  return kDiversifyLazyDefault;
}

// FRECSYS_DPP_FACTOR (read per call; changes no result bit): "ws" keeps the
// factor C in the workspace at every shape; unset: in LDS where it fits
// (dpp_factor_in_lds).
bool dpp_factor_ws(int pool, int k) {
  const char* v = getenv("FRECSYS_DPP_FACTOR");
  return (v && !strcmp(v, "ws")) || !dpp_factor_in_lds(pool, k);
}

// The selection behind pools of `pool` slots on the device, MMR
// (div_select_kernel) or DPP (dpp_select_kernel): div_gram_kernel writes the
// pool Gramians of a sub-batch of `gb` rows, the select kernel reads them, and
// [cnt][k] outputs go to the host.  The Gramians have a sub-batch of their own
// because they are 4 pool^2 bytes a row -- 4 MiB at pool 1024, where they
// would cut the scan of frecsys_recommend_diverse into batches of 59 rows, one
// 64-row block each.  The lazy MMR variant has no Gramian and one sub-batch;
// where the DPP factor does not fit LDS, its 4 k pool bytes lie beside the
// Gramian.
struct PoolStage final : BehindScan {
  const PoolRequest rq;
  const int64_t n;
  const bool dpp, ws;        // the DPP selection; its factor in the workspace
  int64_t gb = 1;
  DiversifyArgs ga{};        // the Gramian launch and the MMR selection
  DppArgs pa{};
  float* d_extra = nullptr;  // the batch's third output row

  // x: lam (MMR; eps unused) or theta (DPP)
  PoolStage(const frecsys_ctx* c, const PoolRequest& r, int64_t rows, int pool, bool is_dpp,
            float x, float eps)
      : rq(r), n(rows), dpp(is_dpp), ws(is_dpp && dpp_factor_ws(pool, r.k)) {
    ga.Y = c->emb[1];
    ga.Dp = c->Dp;
    ga.pool = pa.pool = pool;
    ga.k = pa.k = r.k;
    (dpp ? pa.theta : ga.lam) = x;
    pa.eps = eps;
    (dpp ? pa.raw : ga.raw) = raw();
    ga.lazy = !dpp && diversify_lazy();
  }
  bool raw() const { return (rq.flags & FRECSYS_DIV_RAW_SCORES) != 0; }
  size_t scan_bytes() const override { return (size_t)ga.k * 12; }
  // per row of a sub-batch (0: no sub-batches)
  size_t sub_bytes() const {
    return ga.lazy ? 0 : (size_t)ga.pool * ga.pool * 4 + (ws ? dpp_factor_bytes(ga.pool, ga.k) : 0);
  }
  // nb rows: sub-batches within `budget` bytes (at least one row), the outputs
  void carve_rows(Carver& cv, int64_t nb, size_t budget) {
    const size_t sub = sub_bytes(), k = (size_t)ga.k, P = (size_t)ga.pool;
    gb = sub ? std::min<int64_t>(nb, std::max<int64_t>(1, (int64_t)(budget / sub))) : nb;
    ga.G = cv.take_if<float>(!ga.lazy, (size_t)gb * P * P);
    pa.C = cv.take_if<float>(ws, (size_t)gb * k * P);
    ga.out_items = cv.take<int32_t>((size_t)nb * k);
    ga.out_scores = cv.take<float>((size_t)nb * k);
    d_extra = cv.take_if<float>(rq.extra != nullptr, (size_t)nb * k);
  }
  // behind the scan: outside its per-row budget, within a budget of their own
  void scan_carve(Carver& cv, int64_t nb) override { carve_rows(cv, nb, workspace_budget()); }
  // rows [r0, r0 + cnt) of the call, their pools at ids / pool_scores: per
  // sub-batch two timed launches; the outputs are on their way to the host
  // when it returns (the caller synchronises)
  int run(frecsys_ctx* c, const int32_t* ids, const float* pool_scores, int64_t r0,
          int64_t cnt) override {
    const size_t k = (size_t)ga.k, P = (size_t)ga.pool;
    DiversifyArgs g = ga;
    DppArgs p = pa;
    p.G = ga.G;
    for (int64_t s0 = 0; s0 < cnt; s0 += gb) {
      g.n = p.n = std::min(gb, cnt - s0);
      g.ids = p.ids = ids + (size_t)s0 * P;
      g.pool_scores = p.pool_scores = pool_scores + (size_t)s0 * P;
      g.out_items = p.out_items = ga.out_items + (size_t)s0 * k;
      g.out_scores = p.out_scores = ga.out_scores + (size_t)s0 * k;
      g.out_mmr = p.out_gain = d_extra ? d_extra + (size_t)s0 * k : nullptr;
      if (ga.G) {
        ScopedTimer t(c, "diversify.gram");
        HIP_TRY(c, launch_diversify_gram(g, c->stream));
        t.stop();
      }
      ScopedTimer t(c, dpp ? "dpp.select" : "diversify.select");
      HIP_TRY(c, dpp ? launch_dpp_select(p, c->stream) : launch_diversify_select(g, c->stream));
      t.stop();
    }
    if (!rq.items) return FRECSYS_OK;
    HIP_TRY(c, to_host(c, rq.items + r0 * k, ga.out_items, (size_t)cnt * k));
    HIP_TRY(c, to_host(c, rq.scores + r0 * k, ga.out_scores, (size_t)cnt * k));
    if (rq.extra) HIP_TRY(c, to_host(c, rq.extra + r0 * k, d_extra, (size_t)cnt * k));
    return FRECSYS_OK;
  }
  // flops at the logical dim: the lower triangle of every pool Gramian, then
  // MMR: per step and slot two multiplies and a maximum, a multiply and a
  // subtraction; DPP: the factor's chains, sum over t < k of 2 t pool, every
  // step booked as a DPP step.  Bytes: the pool's item rows gathered once, the
  // Gramian written, k of its rows and the pool read by the selection, the
  // outputs; DPP: the factor written once and read sum over t < k of t pool
  // words; lazy: the norms, then per step one row of products, so the item
  // rows are read k + 1 times
  void book(frecsys_ctx* c) const override {
    const double P = ga.pool, k = ga.k, d = c->dim, out = k * (rq.extra ? 12.0 : 8.0);
    if (dpp)
      add_work(c, "dpp", (double)n * (P * (P + 1.0) * d + k * (k - 1.0) * P),
               (double)n * (P * d * 4.0 + P * P * 4.0 + k * P * 4.0 + P * 8.0 + k * P * 4.0 +
                            k * (k - 1.0) * P * 2.0 + out),
               n);
    else if (ga.lazy)
      add_work(c, "diversify", (double)n * (2.0 * (k + 1.0) * P * d + 5.0 * k * P),
               (double)n * ((k + 1.0) * P * d * 4.0 + P * 8.0 + out), n);
    else
      add_work(c, "diversify", (double)n * (P * (P + 1.0) * d + 5.0 * k * P),
               (double)n * (P * d * 4.0 + P * P * 4.0 + k * P * 4.0 + P * 8.0 + out), n);
  }
};

// frecsys_diversify and frecsys_diversify_dpp behind their first check.  Per
// row of a batch: its pool (ids and scores), its sub-batch bytes and its
// outputs; at least one row per batch, and one sub-batch per batch.
int pools_impl(frecsys_ctx* c, const std::string& w, const int32_t* lists, const float* list_scores,
               PoolStage& st) {
  const int64_t n = st.n;
  const int pool = st.ga.pool;
  if (n < 0) return fail(c, FRECSYS_ERR_INVALID, w + "negative row count");
  if (n == 0) return FRECSYS_OK;
  if (!lists || !list_scores || !st.rq.items || !st.rq.scores)
    return fail(c, FRECSYS_ERR_INVALID, w + "null pointer");
  if (!c->emb[1] || c->n[1] < 1) return fail(c, FRECSYS_ERR_INVALID, w + "no item embeddings");
  const std::string e = pool_error(lists, list_scores, n, pool, c->n[1], st.raw());
  if (!e.empty()) return fail(c, FRECSYS_ERR_INVALID, w + e);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t budget = workspace_budget();
  const size_t per_row = (size_t)pool * 8 + st.sub_bytes() + st.scan_bytes();
  const int64_t nb = std::min<int64_t>(n, std::max<int64_t>(1, (int64_t)(budget / per_row)));
  int32_t* d_ids = nullptr;
  float* d_sc = nullptr;
  int rc = Carver::run(c, [&](Carver& cv) {
    d_ids = cv.take<int32_t>((size_t)nb * pool);
    d_sc = cv.take<float>((size_t)nb * pool);
    st.carve_rows(cv, nb, std::max(budget, (size_t)nb * st.sub_bytes()));
  });
  if (rc) return rc;
  for (int64_t r0 = 0; r0 < n; r0 += nb) {
    const int64_t cnt = std::min(nb, n - r0);
    HIP_TRY(c, to_device(c, d_ids, lists + r0 * pool, (size_t)cnt * pool));
    HIP_TRY(c, to_device(c, d_sc, list_scores + r0 * pool, (size_t)cnt * pool));
    if ((rc = st.run(c, d_ids, d_sc, r0, cnt))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  st.book(c);
  return FRECSYS_OK;
}

// The list quality behind lists of list_k slots that are on the device:
// quality_kernel writes the ILD / novelty rows of a batch, which go to the
// host; exposure_kernel adds the batch's filled slots into counts[nk][items],
// zeroed by upload() and fetched once by finish().  Per row of a batch: the two
// result rows; per call: the cut-offs, the weights and the counts.
struct QualityStage {
  const QualityRequest& rq;
  const int64_t n, m;
  const size_t nk;
  QualityArgs qa{};
  ExposureArgs ea{};

  QualityStage(const frecsys_ctx* c, const QualityRequest& r, int64_t rows, int k)
      : rq(r), n(rows), m(c->n[1]), nk((size_t)r.nk) {
    qa.Y = c->emb[1];
    qa.Dp = c->Dp;
    qa.k = ea.k = k;
    qa.nk = ea.nk = r.nk;
    ea.m = m;
  }
  size_t row_bytes() const { return nk * 8; }
  // per row of a batch, then outside the per-row budget
  void carve(Carver& cv, int64_t nb) {
    qa.ild = cv.take_if<float>(rq.ild != nullptr, (size_t)nb * nk);
    qa.novelty = cv.take_if<float>(rq.novelty != nullptr, (size_t)nb * nk);
    qa.k_list = ea.k_list = cv.take<int32_t>(nk);
    qa.weight = cv.take_if<float>(rq.item_weight != nullptr, (size_t)m);
    ea.counts = cv.take_if<unsigned long long>(rq.exposure != nullptr, nk * (size_t)m);
  }
  int upload(frecsys_ctx* c) {
    HIP_TRY(c, to_device(c, qa.k_list, rq.k_list, nk));
    if (qa.weight) HIP_TRY(c, to_device(c, qa.weight, rq.item_weight, (size_t)m));
    if (ea.counts) HIP_TRY(c, hipMemsetAsync(ea.counts, 0, nk * (size_t)m * 8, c->stream));
    return FRECSYS_OK;
  }
  // rows [r0, r0 + cnt) of the call, their lists at `lists` with list_k slots
  // a row; the result rows are on their way to the host when it returns (the
  // caller synchronises)
  int run(frecsys_ctx* c, const int32_t* lists, int list_k, int64_t r0, int64_t cnt) {
    if (qa.ild || qa.novelty) {
      qa.lists = lists;
      qa.list_k = list_k;
      qa.n = cnt;
      ScopedTimer t(c, "quality");
      HIP_TRY(c, launch_quality(qa, c->stream));
      t.stop();
      if (rq.ild) HIP_TRY(c, to_host(c, rq.ild + r0 * nk, qa.ild, (size_t)cnt * nk));
      if (rq.novelty) HIP_TRY(c, to_host(c, rq.novelty + r0 * nk, qa.novelty, (size_t)cnt * nk));
    }
    if (ea.counts) {
      ea.lists = lists;
      ea.list_k = list_k;
      ea.n = cnt;
      ScopedTimer t(c, "quality.exposure");
      HIP_TRY(c, launch_exposure(ea, c->stream));
      t.stop();
    }
    return FRECSYS_OK;
  }
  // after the last batch: the counts, once per call
  int finish(frecsys_ctx* c) {
    if (!ea.counts) return FRECSYS_OK;
    HIP_TRY(c, to_host(c, reinterpret_cast<unsigned long long*>(rq.exposure), ea.counts,
                       nk * (size_t)m));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FRECSYS_OK;
  }
  // every slot booked as filled.  ILD: per slot two dot products and one axpy
  // over the logical dim; bytes: the slot's padded item row, its id and its
  // weight, the result rows; the exposure's adds are booked as 8 bytes each
  void book(frecsys_ctx* c) const {
    const double k = qa.k, d = c->dim;
    add_work(c, "quality", rq.ild ? (double)n * k * 6.0 * d : 0.0,
             (double)n * (k * ((rq.ild ? c->Dp * 4.0 : 0.0) + 4.0 + (rq.novelty ? 4.0 : 0.0)) +
                          (double)nk * ((rq.ild ? 4.0 : 0.0) + (rq.novelty ? 4.0 : 0.0))) +
                 (rq.exposure ? (double)n * k * (double)nk * 8.0 : 0.0),
             n);
  }
};

// frecsys_rank_quality behind the scan: the selection (with a pool), then the
// metrics (with a ground truth) and the quality of the lists it left.
struct QualityBehind : BehindScan {
  std::optional<PoolStage> ds;
  std::optional<MetricsStage> ms;
  QualityStage qs;

  QualityBehind(const frecsys_ctx* c, const QualityRequest& ql, int64_t n, int list_k)
      : qs(c, ql, n, list_k) {}
  size_t scan_bytes() const override {
    return (ms ? ms->scan_bytes() : 0) + (ds ? ds->scan_bytes() : 0) + qs.row_bytes();
  }
  void scan_carve(Carver& cv, int64_t nb) override {
    if (ms) ms->scan_carve(cv, nb);
    if (ds) ds->scan_carve(cv, nb);
    qs.carve(cv, nb);
  }
  int scan_upload(frecsys_ctx* c) override { return qs.upload(c); }
  int scan_overlap(frecsys_ctx* c) override { return ms ? ms->scan_overlap(c) : FRECSYS_OK; }
  int run(frecsys_ctx* c, const int32_t* lists, const float* scores, int64_t r0,
          int64_t cnt) override {
    int rc;
    if (ds) {
      if ((rc = ds->run(c, lists, scores, r0, cnt))) return rc;
      lists = ds->ga.out_items;
    }
    if (ms && (rc = ms->run(c, lists, nullptr, r0, cnt))) return rc;
    return qs.run(c, lists, qs.qa.k, r0, cnt);
  }
  int finish(frecsys_ctx* c) override {  // the counts, between the stages' work and their own
    if (ms) ms->book(c);
    if (ds) ds->book(c);
    if (int rc = qs.finish(c)) return rc;
    qs.book(c);
    return FRECSYS_OK;
  }
  void no_rows(const frecsys_ctx* c) const override {
    if (qs.rq.exposure)
      std::memset(qs.rq.exposure, 0, sizeof(int64_t) * qs.nk * (size_t)c->n[1]);
  }
};

// The eligibility words and the query row ids of a scan, uploaded.
int upload_query(frecsys_ctx* c, const RecommendArgs& a, const uint8_t* mask, const int64_t* rows,
                 int64_t n) {
  const std::vector<uint32_t> maskw = item_mask_words(a.m, mask);
  HIP_TRY(c, to_device(c, a.maskw, maskw.data(), maskw.size()));
  if (rows) HIP_TRY(c, to_device(c, a.qrows, rows, (size_t)n));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // maskw goes out of scope
  return FRECSYS_OK;
}

// A ranking of the items for n query rows of a side; k is the length of the
// scan's lists (the pool where a selection follows).  scan_impl runs it.
struct ScanCall {
  std::string w;
  int32_t side;
  const int64_t* rows;
  int64_t n;
  int32_t k;
  int32_t flags;
  const uint8_t* item_mask;
  // the timer and work key of the scan, and the scan's launcher: false,
  // rec_scan_kernel (every call but frecsys_recommend_two_stage); true, the
  // bf16 scan of the image in c->d_ts_img, whose bytes are the images'
  const char* key = "recommend";
  bool bf16 = false;
};
// The checks, before any device call (null_outputs is the caller's verdict on
// its own outputs, gt or nullptr a ground truth), the return for zero rows,
// and the device part: the same launch and workspace layout whatever lies
// behind the scan.  A batch's lists and scores stay on the device for `behind`.
int scan_impl(frecsys_ctx* c, const ScanCall& q, bool null_outputs, const MetricsRequest* gt,
              BehindScan& behind) {
  int rc = check_query(c, q.w, q.side, FRECSYS_SIDE_EVAL, &q.k, q.flags, FRECSYS_REC_EXCLUDE_HISTORY);
  if (rc) return rc;
  if (q.n < 0 || (q.n > 0 && null_outputs))
    return fail(c, FRECSYS_ERR_INVALID, q.w + "bad arguments (null outputs)");
  const bool exclude = (q.flags & FRECSYS_REC_EXCLUDE_HISTORY) != 0;
  if ((rc = check_rows(c, q.w, q.side, FRECSYS_SIDE_ITEM, exclude, q.rows, q.n))) return rc;
  const int64_t m = c->n[1], n = q.n;
  if (gt) {
    int32_t mk = 0;
    const std::string e = metric_args_error(n, gt->gt_ptr, gt->gt_items, gt->k_list, gt->nk, m, &mk);
    if (!e.empty()) return fail(c, FRECSYS_ERR_INVALID, q.w + e);
  }
  if (n == 0) {
    behind.no_rows(c);
    return FRECSYS_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // per row of a batch beside the scan's own: history bits, and what is behind
  const ScanPlan p = scan_plan(
      c, q.k, m, n, (exclude ? (size_t)recommend_words(m) * 4 : 0) + behind.scan_bytes());
  c->rec_splits = p.splits;
  RecommendArgs a = scan_args(c, q.side, FRECSYS_SIDE_ITEM, q.k, p.splits, exclude);
  rc = Carver::run(c, [&](Carver& cv) {
    carve_scan(cv, a, p, q.rows != nullptr, n);
    behind.scan_carve(cv, p.nb);
  });
  if (rc) return rc;
  if ((rc = behind.scan_upload(c))) return rc;
  if ((rc = upload_query(c, a, q.item_mask, q.rows, n))) return rc;
  for (int64_t r0 = 0; r0 < n; r0 += p.nb) {  // one timed launch group per row batch
    a.r0 = r0;
    a.n = std::min(p.nb, n - r0);
    ScopedTimer t(c, q.key);
    HIP_TRY(c, q.bf16 ? launch_two_stage_scan(a, c->d_ts_img, c->stream)
                      : launch_recommend(a, c->stream));
    t.mark();
    if (r0 == 0 && (rc = behind.scan_overlap(c))) return rc;
    t.finish();
    if ((rc = behind.run(c, a.out_items, a.out_scores, r0, a.n))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  // scoring flops at the logical dim; bytes: both tables read once (the bf16
  // scan: their images, 2 B a column of the padded width), lists written
  const double dd = c->dim;
  if (q.bf16)
    add_work(c, q.key, 2.0 * (double)n * (double)m * dd,
             ((double)n + (double)m) * two_stage_dh(c->Dp) * 2.0 + (double)n * q.k * 8.0, n);
  else
    add_work(c, q.key, 2.0 * (double)n * (double)m * dd,
             ((double)n + (double)m) * dd * 4.0 + (double)n * q.k * 8.0, n);
  return behind.finish(c);
}

// What frecsys_rank_candidates_metrics and frecsys_sampled_metrics share.
struct CandMetricsCall {
  int32_t side;
  const int64_t* rows;
  int64_t n;
  int32_t flags;
  const uint8_t* item_mask;
  MetricsRequest mt;
  // caller lists (frecsys_rank_candidates_metrics) ...
  const int64_t* cand_ptr;
  const int32_t* cand_items;
  // ... or sampled ones (cand_ptr == nullptr)
  int32_t n_neg;
  uint64_t seed;
  int32_t* neg_count;
  int32_t* negatives;
};

// The argument checks of both, before any device call: frecsys_rank_metrics'
// and frecsys_rank_candidates' cases.  *k = max k_list.
int cand_metrics_check(frecsys_ctx* c, const std::string& w, const CandMetricsCall& q,
                       int32_t* k) {
  int rc = check_query(c, w, q.side, FRECSYS_SIDE_EVAL, nullptr, q.flags,
                       FRECSYS_REC_EXCLUDE_HISTORY);
  if (rc) return rc;
  if (q.n < 0) return fail(c, FRECSYS_ERR_INVALID, w + "negative row count");
  if ((rc = check_cutoffs(c, w, q.mt.k_list, q.mt.nk, k))) return rc;
  if (!q.cand_ptr) {
    if (q.n_neg < 0) return fail(c, FRECSYS_ERR_INVALID, w + "n_neg must not be negative");
    if (q.n_neg > 0 && q.n > INT64_MAX / q.n_neg)
      return fail(c, FRECSYS_ERR_INVALID, w + "n_rows * n_neg overflows");
  }
  if (q.n == 0) return FRECSYS_OK;
  if (!q.mt.recall || !q.mt.ndcg)
    return fail(c, FRECSYS_ERR_INVALID, w + "bad arguments (null outputs)");
  if ((rc = check_rows(c, w, q.side, FRECSYS_SIDE_ITEM,
                       (q.flags & FRECSYS_REC_EXCLUDE_HISTORY) != 0, q.rows, q.n)))
    return rc;
  int32_t mk = 0;
  const std::string e =
      metric_args_error(q.n, q.mt.gt_ptr, q.mt.gt_items, q.mt.k_list, q.mt.nk, c->n[1], &mk);
  if (!e.empty()) return fail(c, FRECSYS_ERR_INVALID, w + e);
  return FRECSYS_OK;
}

// The device part of both: per row batch the candidate ids are uploaded
// (caller lists) or written by the sampling kernels (sampled lists), then
// rank_cand_kernel ranks them where they lie and the metrics stage reads the
// lists where the ranking left them.
int cand_metrics_impl(frecsys_ctx* c, const std::string& w, const CandMetricsCall& q, int32_t k) {
  const bool sampled = q.cand_ptr == nullptr;
  const bool exclude = (q.flags & FRECSYS_REC_EXCLUDE_HISTORY) != 0;
  const int64_t n = q.n, m = c->n[1];
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t budget = workspace_budget();
  const int64_t W = recommend_words(m);
  const bool bits = sampled || exclude;  // one bitmap per row of a batch
  MetricsStage ms(q.mt, n, k);
  // per row of a batch: its outputs, its metric rows, its bitmap -- and its
  // candidate ids.  Sampled lists: the lengths are known only after the pool
  // pass, so rows are cut into batches by the fixed part within half the
  // budget, and each batch into sub-batches whose ids stay within the other
  // half (at least one row each).
  const size_t row_fixed = (size_t)k * 4 + ms.nk * 8 + (bits ? (size_t)W * 4 : 0);
  Cuts ct;
  if (sampled) {
    const int64_t nb =
        std::min<int64_t>(n, std::max<int64_t>(1, (int64_t)((budget / 2) / row_fixed)));
    for (int64_t r0 = 0; r0 < n; r0 += nb) ct.cuts.push_back(std::min(n, r0 + nb));
    ct.max_rows = nb;
  } else {
    ct = cut_by_candidates(q.cand_ptr, n, row_fixed, budget);
  }
  // eligibility bits of the items, and the ascending list of the eligible ids
  // when a mask leaves some out (the domain D of the draws)
  const std::vector<uint32_t> maskw = item_mask_words(m, q.item_mask);
  std::vector<int32_t> dlist;
  int64_t M = m;
  if (sampled && q.item_mask) {
    for (int64_t j = 0; j < m; ++j)
      if (q.item_mask[j]) dlist.push_back((int32_t)j);
    M = (int64_t)dlist.size();
    if (M == m) dlist.clear();
  }
  ms.sort();
  RankCandArgs a = cand_args(c, q.side, k, exclude);
  SampledArgs sa{};
  uint32_t* bitmap = nullptr;
  int rc = Carver::run(c, [&](Carver& cv) {
    a.cand = cv.take<int32_t>((size_t)ct.max_ids);
    bitmap = cv.take_if<uint32_t>(bits, (size_t)ct.max_rows * W);
    a.out_items = cv.take<int32_t>((size_t)ct.max_rows * k);
    ms.carve_rows(cv, ct.max_rows);
    // outside the per-row budget: per call
    a.maskw = cv.take<uint32_t>((size_t)W);
    a.cand_ptr = cv.take<int64_t>((size_t)n + 1);
    a.qrows = cv.take_if<int64_t>(q.rows != nullptr, (size_t)n);
    ms.carve_inputs(cv, ms.sg.size());
    sa.pool = cv.take<int32_t>(sampled ? (size_t)n : 0);
    sa.dlist = cv.take_if<int32_t>(!dlist.empty(), dlist.size());
  });
  if (rc) return rc;
  a.bitmap = exclude ? bitmap : nullptr;
  HIP_TRY(c, to_device(c, a.maskw, maskw.data(), maskw.size()));
  if (q.rows) HIP_TRY(c, to_device(c, a.qrows, q.rows, (size_t)n));
  if (!sampled) HIP_TRY(c, to_device(c, a.cand_ptr, q.cand_ptr, (size_t)n + 1));
  if (!dlist.empty()) HIP_TRY(c, to_device(c, sa.dlist, dlist.data(), dlist.size()));
  if ((rc = ms.upload(c))) return rc;
  if (sampled)
    HIP_TRY(c, hipMemsetAsync(c->d_fail, 0xFF, sizeof(unsigned long long), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // ranks and scores rows [s0, s1) of the call from the ids at a.cand
  auto rank_rows = [&](int64_t s0, int64_t s1, int64_t cand_base) -> int {
    a.r0 = s0;
    a.n = s1 - s0;
    a.cand_base = cand_base;
    {
      ScopedTimer t(c, "rank_candidates");
      HIP_TRY(c, launch_rank_candidates(a, c->stream));
      t.stop();
    }
    return ms.run(c, a.out_items, nullptr, s0, a.n);
  };
  double pairs = 0.0;
  if (!sampled) {
    for (size_t b = 0; b + 1 < ct.cuts.size(); ++b) {
      const int64_t s0 = ct.cuts[b], s1 = ct.cuts[b + 1];
      const int64_t base = q.cand_ptr[s0], ids = q.cand_ptr[s1] - base;
      if (ids > 0) HIP_TRY(c, to_device(c, a.cand, q.cand_items + base, (size_t)ids));
      if ((rc = rank_rows(s0, s1, base))) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    pairs = (double)q.cand_ptr[n];
  } else {
    sa.qrows = a.qrows;
    sa.m = m;
    sa.W = W;
    sa.row_ptr = a.row_ptr;
    sa.col = a.col;
    sa.maskw = a.maskw;
    sa.M = M;
    sa.gt_ptr = ms.ma.gt_ptr;
    sa.gt = ms.ma.gt;
    sa.n_neg = q.n_neg;
    sa.seed = q.seed;
    sa.cand_ptr = a.cand_ptr;
    sa.fail = c->d_fail;
    const std::vector<int64_t>& gt_sp = ms.sp;
    std::vector<int32_t> pool((size_t)ct.max_rows), ids_host;
    std::vector<int64_t> ptr((size_t)ct.max_rows + 1);
    for (size_t b = 0; b + 1 < ct.cuts.size(); ++b) {
      const int64_t b0 = ct.cuts[b], b1 = ct.cuts[b + 1], nb = b1 - b0;
      sa.r0 = b0;
      sa.n = nb;
      sa.bitmap = bitmap;
      {
        ScopedTimer t(c, "sample_negatives");
        HIP_TRY(c, launch_sampled_pool(sa, c->stream));
        t.stop();
      }
      HIP_TRY(c, to_host(c, pool.data(), sa.pool + b0, (size_t)nb));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      // list i of the batch lies at ptr[i - b0] (ptr[0] = 0), on the device
      // at entry i of the call's pointer array
      ptr[0] = 0;
      for (int64_t i = 0; i < nb; ++i) {
        const int64_t E = pool[(size_t)i];
        const int64_t cnt = whole_pool_row(q.n_neg, E, M) ? E : q.n_neg;
        if (q.neg_count) q.neg_count[b0 + i] = (int32_t)cnt;
        ptr[(size_t)i + 1] =
            ptr[(size_t)i] + (gt_sp[(size_t)(b0 + i) + 1] - gt_sp[(size_t)(b0 + i)]) + cnt;
      }
      HIP_TRY(c, to_device(c, a.cand_ptr + b0, ptr.data(), (size_t)nb + 1));
      pairs += (double)ptr[(size_t)nb];
      for (int64_t s0 = b0; s0 < b1;) {
        int64_t s1 = s0 + 1;
        const int64_t base = ptr[(size_t)(s0 - b0)];
        while (s1 < b1 && (size_t)(ptr[(size_t)(s1 + 1 - b0)] - base) * 4 <= budget / 2) ++s1;
        const int64_t ids = ptr[(size_t)(s1 - b0)] - base;
        if ((rc = ensure(c, c->d_samp_ids, (size_t)std::max<int64_t>(ids, 1)))) return rc;
        sa.r0 = s0;
        sa.n = s1 - s0;
        sa.bitmap = bitmap + (size_t)(s0 - b0) * W;
        sa.cand_base = base;
        sa.cand = c->d_samp_ids;
        {
          ScopedTimer t(c, "sample_negatives");
          HIP_TRY(c, launch_sampled_fill(sa, c->stream));
          t.stop();
        }
        if (q.negatives && q.n_neg > 0) {
          ids_host.resize((size_t)ids);
          HIP_TRY(c, to_host(c, ids_host.data(), sa.cand, (size_t)ids));
        }
        a.cand = sa.cand;
        a.bitmap = exclude ? sa.bitmap : nullptr;  // refilled with the history alone
        if ((rc = rank_rows(s0, s1, base))) return rc;
        unsigned long long f = ~0ull;
        HIP_TRY(c, hipMemcpyAsync(&f, c->d_fail, sizeof(f), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (f != ~0ull)
          return fail(c, FRECSYS_ERR_HIP,
                      w + "the draws of query row " + std::to_string((int64_t)f - 1) +
                          " reached the cap");
        if (q.negatives && q.n_neg > 0)
          for (int64_t i = s0; i < s1; ++i) {
            int32_t* out = q.negatives + i * q.n_neg;
            const int64_t g = gt_sp[(size_t)i + 1] - gt_sp[(size_t)i];
            if (whole_pool_row(q.n_neg, pool[(size_t)(i - b0)], M))
              std::fill(out, out + q.n_neg, -1);
            else
              std::memcpy(out, ids_host.data() + (ptr[(size_t)(i - b0)] - base) + g,
                          sizeof(int32_t) * (size_t)q.n_neg);
          }
        s0 = s1;
      }
    }
    // bytes: every row's bitmap zeroed, then read by the pool pass; the ids
    // of the lists written
    add_work(c, "sample_negatives", 0.0, (double)n * (double)W * 8.0 + pairs * 4.0, n);
  }
  // as frecsys_rank_candidates (the lists: ids only) and frecsys_rank_metrics
  add_work(c, "rank_candidates", 2.0 * pairs * c->dim,
           pairs * c->Dp * 4.0 + pairs * 4.0 + (double)n * k * 4.0, n);
  ms.book(c);
  return FRECSYS_OK;
}

}  // namespace

extern "C" {

int frecsys_recommend(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows, int32_t k,
                      int32_t flags, const uint8_t* item_mask, int32_t* items, float* scores) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "recommend: null context");
  ListsOut out(items, scores, k);
  return scan_impl(c, {"recommend: ", side, rows, n_rows, k, flags, item_mask}, !items, nullptr,
                   out);
}

int frecsys_recommend_two_stage(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                                int32_t k, int32_t pool, int32_t flags, const uint8_t* item_mask,
                                int32_t* items, float* scores, uint8_t* certified,
                                int32_t* pool_items, float* pool_scores) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "recommend_two_stage: null context");
  const std::string w = "recommend_two_stage: ";
  if (pool == 0) {  // the default: the 4 k of the re-ranking calls, at least 64
    if (k < 1 || k > 1024) return fail(c, FRECSYS_ERR_INVALID, w + "k must be in [1, 1024]");
    pool = std::min(1024, std::max(64, 4 * k));
  }
  if (int rc = check_diversify(c, w, k, pool, 0.0f, flags,
                               FRECSYS_REC_EXCLUDE_HISTORY | FRECSYS_TS_EXACT))
    return rc;
  const int32_t scan_flags = flags & FRECSYS_REC_EXCLUDE_HISTORY;
  TwoStageStage st(c, side, rows, n_rows, k, pool, items, scores, pool_items, pool_scores);
  ScanCall q{w, side, rows, n_rows, pool, scan_flags, item_mask};
  q.key = "two_stage.scan";
  q.bf16 = true;
  int rc = scan_impl(c, q, !items, nullptr, st);
  if (rc || n_rows == 0) return rc;
  // the rows stage 2 could not certify: re-run by the exact scan, if asked for
  std::vector<int64_t> again, at;
  for (int64_t i = 0; i < n_rows; ++i) {
    if (st.cert[(size_t)i]) {
      ++c->ts_certified;
    } else if (flags & FRECSYS_TS_EXACT) {
      again.push_back(rows ? rows[i] : i);
      at.push_back(i);
      st.cert[(size_t)i] = 2;
    }
  }
  if (!again.empty()) {
    const size_t na = again.size(), kk = (size_t)k;
    std::vector<int32_t> fi(na * kk);
    std::vector<float> fs(scores ? na * kk : 0);
    ListsOut out(fi.data(), scores ? fs.data() : nullptr, k);
    ScanCall fq{w, side, again.data(), (int64_t)na, k, scan_flags, item_mask};
    fq.key = "two_stage.fallback";
    if ((rc = scan_impl(c, fq, false, nullptr, out))) return rc;
    for (size_t j = 0; j < na; ++j) {
      std::memcpy(items + (size_t)at[j] * kk, fi.data() + j * kk, kk * sizeof(int32_t));
      if (scores) std::memcpy(scores + (size_t)at[j] * kk, fs.data() + j * kk, kk * sizeof(float));
    }
    c->ts_fallback_rows += (int64_t)na;
  }
  if (certified) std::memcpy(certified, st.cert.data(), (size_t)n_rows);
  return FRECSYS_OK;
}

int frecsys_rank_metrics(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                         int32_t flags, const uint8_t* item_mask, const int64_t* gt_ptr,
                         const int32_t* gt_items, const int32_t* k_list, int32_t nk, float* recall,
                         float* ndcg) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "rank_metrics: null context");
  int32_t k = 0;  // the list length is the largest cut-off
  if (int rc = check_cutoffs(c, "rank_metrics: ", k_list, nk, &k)) return rc;
  const MetricsRequest mt{gt_ptr, gt_items, k_list, nk, recall, ndcg};
  MetricsStage ms(mt, n_rows, k);
  return scan_impl(c, {"rank_metrics: ", side, rows, n_rows, k, flags, item_mask},
                   !recall || !ndcg, &mt, ms);
}

int frecsys_recommend_diverse(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                              int32_t k, int32_t pool, float lam, int32_t flags,
                              const uint8_t* item_mask, int32_t* items, float* scores,
                              float* mmr) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "recommend_diverse: null context");
  const std::string w = "recommend_diverse: ";
  if (int rc = check_diversify(c, w, k, pool, lam, flags,
                               FRECSYS_REC_EXCLUDE_HISTORY | FRECSYS_DIV_RAW_SCORES))
    return rc;
  PoolStage ds(c, {k, flags, items, scores, mmr}, n_rows, pool, /*dpp=*/false, lam, 0.0f);
  return scan_impl(c, {w, side, rows, n_rows, pool, flags & FRECSYS_REC_EXCLUDE_HISTORY, item_mask},
                   !items || !scores, nullptr, ds);
}

int frecsys_diversify(frecsys_ctx* c, const int32_t* lists, const float* list_scores, int64_t n,
                      int32_t pool, int32_t k, float lam, int32_t flags, int32_t* items,
                      float* scores, float* mmr) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "diversify: null context");
  const std::string w = "diversify: ";
  if (int rc = check_diversify(c, w, k, pool, lam, flags, FRECSYS_DIV_RAW_SCORES)) return rc;
  PoolStage ds(c, {k, flags, items, scores, mmr}, n, pool, /*dpp=*/false, lam, 0.0f);
  return pools_impl(c, w, lists, list_scores, ds);
}

int frecsys_recommend_dpp(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                          int32_t k, int32_t pool, float theta, float eps, int32_t flags,
                          const uint8_t* item_mask, int32_t* items, float* scores, float* gain) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "recommend_dpp: null context");
  const std::string w = "recommend_dpp: ";
  if (int rc = check_dpp(c, w, k, pool, theta, eps, flags,
                         FRECSYS_REC_EXCLUDE_HISTORY | FRECSYS_DIV_RAW_SCORES))
    return rc;
  PoolStage ps(c, {k, flags, items, scores, gain}, n_rows, pool, /*dpp=*/true, theta, eps);
  return scan_impl(c, {w, side, rows, n_rows, pool, flags & FRECSYS_REC_EXCLUDE_HISTORY, item_mask},
                   !items || !scores, nullptr, ps);
}

int frecsys_diversify_dpp(frecsys_ctx* c, const int32_t* lists, const float* list_scores,
                          int64_t n, int32_t pool, int32_t k, float theta, float eps,
                          int32_t flags, int32_t* items, float* scores, float* gain) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "diversify_dpp: null context");
  const std::string w = "diversify_dpp: ";
  if (int rc = check_dpp(c, w, k, pool, theta, eps, flags, FRECSYS_DIV_RAW_SCORES)) return rc;
  PoolStage ps(c, {k, flags, items, scores, gain}, n, pool, /*dpp=*/true, theta, eps);
  return pools_impl(c, w, lists, list_scores, ps);
}

int frecsys_rank_quality(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                         int32_t flags, const uint8_t* item_mask, const int32_t* k_list,
                         int32_t nk, int32_t pool, float lam, int32_t div_flags,
                         const float* item_weight, const int64_t* gt_ptr, const int32_t* gt_items,
                         float* ild, float* novelty, float* recall, float* ndcg,
                         int64_t* exposure) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "rank_quality: null context");
  const std::string w = "rank_quality: ";
  const QualityRequest ql{k_list, nk, item_weight, ild, novelty, exposure};
  std::string e = quality_args_error(ql, kMetricMaxK, c->n[1], recall || ndcg);
  if (e.empty() && !gt_ptr && (recall || ndcg)) e = "recall / ndcg need a ground truth";
  if (e.empty() && gt_ptr && (!recall || !ndcg)) e = "a ground truth needs recall and ndcg";
  if (!e.empty()) return fail(c, FRECSYS_ERR_INVALID, w + e);
  const int32_t k = max_cutoff(k_list, nk);  // the list length is the largest cut-off
  if (pool != 0) {
    if (int rc = check_diversify(c, w, k, pool, lam, div_flags, FRECSYS_DIV_RAW_SCORES)) return rc;
  } else if (div_flags != 0) {
    return fail(c, FRECSYS_ERR_INVALID, w + "div_flags without a pool");
  }
  if (n_rows < 0) return fail(c, FRECSYS_ERR_INVALID, w + "negative row count");
  const MetricsRequest mt{gt_ptr, gt_items, k_list, nk, recall, ndcg};
  // every stage reads lists of k slots: the selection's, else the scan's
  QualityBehind behind(c, ql, n_rows, k);
  if (pool)
    behind.ds.emplace(c, PoolRequest{k, div_flags, nullptr, nullptr, nullptr}, n_rows, pool, false,
                      lam, 0.0f);
  if (gt_ptr) behind.ms.emplace(mt, n_rows, k);
  return scan_impl(c, {w, side, rows, n_rows, pool ? pool : k, flags, item_mask}, false,
                   gt_ptr ? &mt : nullptr, behind);
}

int frecsys_lists_quality(frecsys_ctx* c, const int32_t* lists, int64_t n, int32_t list_k,
                          const int32_t* k_list, int32_t nk, const float* item_weight, float* ild,
                          float* novelty, int64_t* exposure) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "lists_quality: null context");
  const std::string w = "lists_quality: ";
  if (list_k < 1) return fail(c, FRECSYS_ERR_INVALID, w + "list_k must be positive");
  if (!c->emb[1] || c->n[1] < 1) return fail(c, FRECSYS_ERR_INVALID, w + "no item embeddings");
  const int64_t m = c->n[1];
  const QualityRequest ql{k_list, nk, item_weight, ild, novelty, exposure};
  std::string e = quality_args_error(ql, std::min<int32_t>(kMetricMaxK, list_k), m, false);
  if (e.empty()) e = lists_error(lists, n, list_k, m);
  if (!e.empty()) return fail(c, FRECSYS_ERR_INVALID, w + e);
  if (n == 0) {
    if (exposure) std::memset(exposure, 0, sizeof(int64_t) * (size_t)nk * (size_t)m);
    return FRECSYS_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  QualityStage qs(c, ql, n, max_cutoff(k_list, nk));
  // per row of a batch: its list and its result rows; at least one row per batch
  const size_t per_row = (size_t)list_k * 4 + qs.row_bytes();
  const int64_t nb =
      std::min<int64_t>(n, std::max<int64_t>(1, (int64_t)(workspace_budget() / per_row)));
  int32_t* d_lists = nullptr;
  int rc = Carver::run(c, [&](Carver& cv) {
    d_lists = cv.take<int32_t>((size_t)nb * list_k);
    qs.carve(cv, nb);
  });
  if (rc) return rc;
  if ((rc = qs.upload(c))) return rc;
  for (int64_t r0 = 0; r0 < n; r0 += nb) {
    const int64_t cnt = std::min(nb, n - r0);
    HIP_TRY(c, to_device(c, d_lists, lists + r0 * list_k, (size_t)cnt * list_k));
    if ((rc = qs.run(c, d_lists, list_k, r0, cnt))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if ((rc = qs.finish(c))) return rc;
  qs.book(c);
  return FRECSYS_OK;
}

int frecsys_score_pairs(frecsys_ctx* c, int32_t side, const int64_t* rows, const int32_t* items,
                        int64_t n_pairs, float* scores) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "score_pairs: null context");
  const std::string w = "score_pairs: ";
  int rc = check_query(c, w, side, FRECSYS_SIDE_EVAL, nullptr, 0, 0);
  if (rc) return rc;
  if (n_pairs < 0) return fail(c, FRECSYS_ERR_INVALID, w + "negative pair count");
  if (n_pairs == 0) return FRECSYS_OK;
  if (!rows || !items || !scores) return fail(c, FRECSYS_ERR_INVALID, w + "null pointer");
  if (!c->emb[side] || !c->emb[1])
    return fail(c, FRECSYS_ERR_INVALID, w + "side has no embeddings yet");
  const int64_t ns = c->n[side], m = c->n[1], n = n_pairs;
  for (int64_t i = 0; i < n; ++i) {  // pair by pair: the first bad pair is the one reported
    if (rows[i] < 0 || rows[i] >= ns)
      return fail(c, FRECSYS_ERR_INVALID, w + "row id " + std::to_string(rows[i]) + " out of range");
    if (items[i] < 0 || items[i] >= m)
      return fail(c, FRECSYS_ERR_INVALID,
                  w + "item id " + std::to_string(items[i]) + " out of range");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // per pair: row id, item id, score
  const int64_t nb = std::min<int64_t>(n, std::max<int64_t>(64, (int64_t)(workspace_budget() / 16)));
  ScorePairsArgs a{};
  a.X = c->emb[side];
  a.Y = c->emb[1];
  a.Dp = c->Dp;
  rc = Carver::run(c, [&](Carver& cv) {
    a.rows = cv.take<int64_t>((size_t)nb);
    a.items = cv.take<int32_t>((size_t)nb);
    a.out = cv.take<float>((size_t)nb);
  });
  if (rc) return rc;
  for (int64_t p0 = 0; p0 < n; p0 += nb) {  // one timed launch per pair batch
    a.n = std::min(nb, n - p0);
    HIP_TRY(c, to_device(c, a.rows, rows + p0, (size_t)a.n));
    HIP_TRY(c, to_device(c, a.items, items + p0, (size_t)a.n));
    ScopedTimer t(c, "score_pairs");
    HIP_TRY(c, launch_score_pairs(a, c->stream));
    t.stop();
    HIP_TRY(c, to_host(c, scores + p0, a.out, (size_t)a.n));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  // flops at the logical dim; bytes: one padded item row per pair, ids, scores
  add_work(c, "score_pairs", 2.0 * (double)n * c->dim,
           (double)n * c->Dp * 4.0 + (double)n * 12.0 + (double)n * 4.0, n);
  return FRECSYS_OK;
}

int frecsys_rank_candidates(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                            const int64_t* cand_ptr, const int32_t* cand_items, int32_t k,
                            int32_t flags, const uint8_t* item_mask, int32_t* items,
                            float* scores) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "rank_candidates: null context");
  const std::string w = "rank_candidates: ";
  int rc = check_query(c, w, side, FRECSYS_SIDE_EVAL, &k, flags, FRECSYS_REC_EXCLUDE_HISTORY);
  if (rc) return rc;
  if (n_rows < 0) return fail(c, FRECSYS_ERR_INVALID, w + "negative row count");
  if (n_rows == 0) return FRECSYS_OK;
  if (!cand_ptr || !items) return fail(c, FRECSYS_ERR_INVALID, w + "null pointer");
  const bool exclude = (flags & FRECSYS_REC_EXCLUDE_HISTORY) != 0;
  const int64_t m = c->n[1], n = n_rows;
  if ((rc = check_rows(c, w, side, FRECSYS_SIDE_ITEM, exclude, rows, n))) return rc;
  if ((rc = check_candidates(c, w, cand_ptr, cand_items, n, m))) return rc;
  const int64_t pairs = cand_ptr[n];
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t W = recommend_words(m);
  // per row of a batch: its candidate ids, its outputs, its history bits
  const Cuts ct = cut_by_candidates(cand_ptr, n, (size_t)k * 8 + (exclude ? (size_t)W * 4 : 0),
                                    workspace_budget());
  RankCandArgs a = cand_args(c, side, k, exclude);
  rc = Carver::run(c, [&](Carver& cv) {
    a.cand = cv.take<int32_t>((size_t)ct.max_ids);
    a.bitmap = cv.take_if<uint32_t>(exclude, (size_t)ct.max_rows * W);
    a.out_items = cv.take<int32_t>((size_t)ct.max_rows * k);
    a.out_scores = cv.take<float>((size_t)ct.max_rows * k);
    a.maskw = cv.take<uint32_t>((size_t)W);
    a.cand_ptr = cv.take<int64_t>((size_t)n + 1);
    a.qrows = cv.take_if<int64_t>(rows != nullptr, (size_t)n);
  });
  if (rc) return rc;
  if (!scores) a.out_scores = nullptr;
  const std::vector<uint32_t> maskw = item_mask_words(m, item_mask);
  HIP_TRY(c, to_device(c, a.maskw, maskw.data(), maskw.size()));
  HIP_TRY(c, to_device(c, a.cand_ptr, cand_ptr, (size_t)n + 1));
  if (rows) HIP_TRY(c, to_device(c, a.qrows, rows, (size_t)n));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t b = 0; b + 1 < ct.cuts.size(); ++b) {  // one timed launch group per row batch
    a.r0 = ct.cuts[b];
    a.n = ct.cuts[b + 1] - ct.cuts[b];
    a.cand_base = cand_ptr[a.r0];
    const int64_t ids = cand_ptr[a.r0 + a.n] - a.cand_base;
    if (ids > 0) HIP_TRY(c, to_device(c, a.cand, cand_items + a.cand_base, (size_t)ids));
    ScopedTimer t(c, "rank_candidates");
    HIP_TRY(c, launch_rank_candidates(a, c->stream));
    t.stop();
    if ((rc = copy_lists(c, items, scores, k, a.r0, a.n, a.out_items, a.out_scores))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  // flops at the logical dim; bytes: one padded item row per candidate, the
  // ids read, the lists written
  add_work(c, "rank_candidates", 2.0 * (double)pairs * c->dim,
           (double)pairs * c->Dp * 4.0 + (double)pairs * 4.0 + (double)n * k * 8.0, n);
  return FRECSYS_OK;
}

int frecsys_rank_candidates_metrics(frecsys_ctx* c, int32_t side, const int64_t* rows,
                                    int64_t n_rows, const int64_t* cand_ptr,
                                    const int32_t* cand_items, int32_t flags,
                                    const uint8_t* item_mask, const int64_t* gt_ptr,
                                    const int32_t* gt_items, const int32_t* k_list, int32_t nk,
                                    float* recall, float* ndcg) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "rank_candidates_metrics: null context");
  const std::string w = "rank_candidates_metrics: ";
  if (!cand_ptr && n_rows != 0) return fail(c, FRECSYS_ERR_INVALID, w + "null cand_ptr");
  static const int64_t kNoLists[1] = {0};
  const CandMetricsCall q{side, rows, n_rows, flags, item_mask,
                          MetricsRequest{gt_ptr, gt_items, k_list, nk, recall, ndcg},
                          cand_ptr ? cand_ptr : kNoLists, cand_items, 0, 0, nullptr, nullptr};
  int32_t k = 0;
  int rc = cand_metrics_check(c, w, q, &k);
  if (rc || n_rows == 0) return rc;
  if ((rc = check_candidates(c, w, cand_ptr, cand_items, n_rows, c->n[1]))) return rc;
  return cand_metrics_impl(c, w, q, k);
}

int frecsys_sampled_metrics(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                            int32_t flags, const uint8_t* item_mask, const int64_t* gt_ptr,
                            const int32_t* gt_items, int32_t n_neg, uint64_t seed,
                            const int32_t* k_list, int32_t nk, float* recall, float* ndcg,
                            int32_t* neg_count, int32_t* negatives) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "sampled_metrics: null context");
  const std::string w = "sampled_metrics: ";
  const CandMetricsCall q{side, rows, n_rows, flags, item_mask,
                          MetricsRequest{gt_ptr, gt_items, k_list, nk, recall, ndcg},
                          nullptr, nullptr, n_neg, seed, neg_count, negatives};
  int32_t k = 0;
  const int rc = cand_metrics_check(c, w, q, &k);
  if (rc || n_rows == 0) return rc;
  return cand_metrics_impl(c, w, q, k);
}

int frecsys_similar(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows, int32_t k,
                    int32_t flags, const uint8_t* mask, int32_t* ids, float* scores) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "similar: null context");
  const std::string w = "similar: ";
  int rc = check_query(c, w, side, FRECSYS_SIDE_ITEM, &k, flags,
                       FRECSYS_SIM_COSINE | FRECSYS_SIM_KEEP_SELF);
  if (rc) return rc;
  if (n_rows < 0 || (n_rows > 0 && !ids))
    return fail(c, FRECSYS_ERR_INVALID, w + "bad arguments (null outputs)");
  // ("no embeddings" cannot happen today: a context allocates the USER and
  // ITEM tables when it is created; kept for the day a table is allocated
  // lazily)
  if ((rc = check_rows(c, w, side, side, false, rows, n_rows))) return rc;
  const int64_t m = c->n[side], n = n_rows;
  if (n == 0) return FRECSYS_OK;
  const bool cosine = (flags & FRECSYS_SIM_COSINE) != 0;
  HIP_TRY(c, hipSetDevice(c->device));
  // frecsys_recommend's scan of the side's own table (no history bitmap: the
  // one excluded id of a row is tested in the scan).  Not scan_impl: table, norm
  // pass, inv / skip_self, timer, work and splits counter would be six parameters.
  const ScanPlan p = scan_plan(c, k, m, n, 0);
  RecommendArgs a = scan_args(c, side, side, k, p.splits, false);
  if ((rc = Carver::run(c, [&](Carver& cv) { carve_scan(cv, a, p, rows != nullptr, n); })))
    return rc;
  // outside the per-row budget: one inverse norm per row of the side
  if (cosine && (rc = ensure(c, c->d_sim_inv, (size_t)m))) return rc;
  if ((rc = upload_query(c, a, mask, rows, n))) return rc;
  if (cosine) {  // per call: every solve rewrites the table
    ScopedTimer t(c, "similar.norms");
    HIP_TRY(c, launch_row_inv_norm(c->emb[side], m, c->Dp, c->d_sim_inv, c->stream));
    t.stop();
  }
  a.inv = cosine ? (const float*)c->d_sim_inv : nullptr;
  a.skip_self = (flags & FRECSYS_SIM_KEEP_SELF) ? 0 : 1;
  for (int64_t r0 = 0; r0 < n; r0 += p.nb) {  // one timed launch group per row batch
    a.r0 = r0;
    a.n = std::min(p.nb, n - r0);
    ScopedTimer t(c, "similar");
    HIP_TRY(c, launch_recommend(a, c->stream));
    t.stop();
    if ((rc = copy_lists(c, ids, scores, k, r0, a.n, a.out_items, a.out_scores))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  // scoring flops at the logical dim; bytes: the queries and the table read,
  // the table once more by the norm pass, the lists written
  const double dd = c->dim;
  add_work(c, "similar", 2.0 * (double)n * (double)m * dd,
           ((double)n + (cosine ? 2.0 : 1.0) * (double)m) * dd * 4.0 + (double)n * k * 8.0, n);
  return FRECSYS_OK;
}

int frecsys_audience(frecsys_ctx* c, const int64_t* items, int64_t n_items, int32_t k,
                     int32_t flags, const uint8_t* user_mask, int32_t* users, float* scores) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "audience: null context");
  const std::string w = "audience: ";
  int rc = check_query(c, w, FRECSYS_SIDE_USER, FRECSYS_SIDE_ITEM, &k, flags,
                       FRECSYS_AUD_EXCLUDE_HISTORY);
  if (rc) return rc;
  if (n_items < 0 || (n_items > 0 && !users))
    return fail(c, FRECSYS_ERR_INVALID, w + "bad arguments (null outputs)");
  const bool exclude = (flags & FRECSYS_AUD_EXCLUDE_HISTORY) != 0;
  if ((rc = check_rows(c, w, FRECSYS_SIDE_ITEM, FRECSYS_SIDE_USER, exclude, items, n_items)))
    return rc;
  const int64_t m = c->n[FRECSYS_SIDE_USER], n = n_items;
  if (n == 0) return FRECSYS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  int dev_cus = 256;
  (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c->device);
  frecsys_audience_plan_t pl;
  if ((rc = frecsys_audience_plan(c->dim, m, n, k, std::max(1, dev_cus), exclude ? 1 : 0, &pl)))
    return fail(c, rc, w + "no plan for this shape");
  c->rec_splits = pl.splits;
  const int64_t nb = pl.rows_per_batch;
  const std::vector<uint32_t> maskw = item_mask_words(m, user_mask);
  if (pl.thin) {
    // the thin-query kernel: per query of a batch its lists per split, what the
    // first reduce round leaves, the history bits and the outputs
    AudienceArgs a{};
    a.X = c->emb[FRECSYS_SIDE_ITEM];
    a.Y = c->emb[FRECSYS_SIDE_USER];
    a.m = m;
    a.Dp = c->Dp;
    a.k = k;
    a.splits = pl.splits;
    a.row_ptr = exclude ? c->rp[FRECSYS_SIDE_ITEM] : nullptr;
    a.col = exclude ? c->col[FRECSYS_SIDE_ITEM] : nullptr;
    const size_t red = (size_t)audience_reduce_lists(pl.splits, k);
    rc = Carver::run(c, [&](Carver& cv) {
      a.cand = cv.take<unsigned long long>((size_t)nb * pl.splits * pl.slots);
      a.counts = cv.take<int32_t>((size_t)nb * pl.splits);
      a.red = cv.take_if<unsigned long long>(red > 0, (size_t)nb * red * k);
      a.red_counts = cv.take_if<int32_t>(red > 0, (size_t)nb * red);
      a.bitmap = cv.take_if<uint32_t>(exclude, (size_t)nb * maskw.size());
      a.out_items = cv.take<int32_t>((size_t)nb * k);
      a.out_scores = cv.take<float>((size_t)nb * k);
      a.maskw = cv.take<uint32_t>(maskw.size());
      a.qrows = cv.take_if<int64_t>(items != nullptr, (size_t)n);
    });
    if (rc) return rc;
    HIP_TRY(c, to_device(c, a.maskw, maskw.data(), maskw.size()));
    if (items) HIP_TRY(c, to_device(c, a.qrows, items, (size_t)n));
    for (int64_t r0 = 0; r0 < n; r0 += nb) {  // one timed launch group per query batch
      a.r0 = r0;
      a.n = std::min(nb, n - r0);
      ScopedTimer t(c, "audience");
      HIP_TRY(c, launch_audience_thin(a, c->stream));
      t.stop();
      if ((rc = copy_lists(c, users, scores, k, r0, a.n, a.out_items, a.out_scores))) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
  } else {
    // frecsys_recommend's scan, the item rows as queries and the user table
    // searched: the plan is scan_plan's arithmetic
    const ScanPlan p{pl.splits, pl.slots, nb};
    RecommendArgs a = scan_args(c, FRECSYS_SIDE_ITEM, FRECSYS_SIDE_USER, k, p.splits, exclude);
    if ((rc = Carver::run(c, [&](Carver& cv) { carve_scan(cv, a, p, items != nullptr, n); })))
      return rc;
    HIP_TRY(c, to_device(c, a.maskw, maskw.data(), maskw.size()));
    if (items) HIP_TRY(c, to_device(c, a.qrows, items, (size_t)n));
    for (int64_t r0 = 0; r0 < n; r0 += nb) {  // one timed launch group per row batch
      a.r0 = r0;
      a.n = std::min(nb, n - r0);
      ScopedTimer t(c, "audience");
      HIP_TRY(c, launch_recommend(a, c->stream));
      t.stop();
      if ((rc = copy_lists(c, users, scores, k, r0, a.n, a.out_items, a.out_scores))) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
  }
  // scoring flops at the logical dim; bytes: the user table once per pass, the
  // queries, the lists written
  add_work(c, "audience", 2.0 * (double)n * (double)m * (double)c->dim,
           ((double)pl.passes * (double)m + (double)n) * c->Dp * 4.0 + (double)n * k * 8.0, n);
  return FRECSYS_OK;
}

int frecsys_rank_positions(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                           int32_t flags, const uint8_t* item_mask, const int64_t* gt_ptr,
                           const int32_t* gt_items, int32_t* rank, int32_t* eligible, float* mrr,
                           float* auc) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "rank_positions: null context");
  const std::string w = "rank_positions: ";
  int rc = check_query(c, w, side, FRECSYS_SIDE_EVAL, nullptr, flags, FRECSYS_REC_EXCLUDE_HISTORY);
  if (rc) return rc;
  if (n_rows < 0 || (n_rows > 0 && !rank && !eligible && !mrr && !auc))
    return fail(c, FRECSYS_ERR_INVALID, w + "bad arguments (null outputs)");
  const bool exclude = (flags & FRECSYS_REC_EXCLUDE_HISTORY) != 0;
  if ((rc = check_rows(c, w, side, FRECSYS_SIDE_ITEM, exclude, rows, n_rows))) return rc;
  const int64_t m = c->n[1], n = n_rows;
  {
    const int32_t one = 1;  // the ground-truth cases of the metric calls; no cut-offs here
    int32_t mk = 0;
    const std::string e = metric_args_error(n, gt_ptr, gt_items, &one, 1, m, &mk);
    if (!e.empty()) return fail(c, FRECSYS_ERR_INVALID, w + e);
  }
  if (n == 0) return FRECSYS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t W = recommend_words(m);
  // per ground-truth entry of a batch: id, word, threshold, counter, rank; per
  // row: one more counter, the threshold count, eligible, mrr, auc, history bits
  const Cuts ct = cut_by_candidates(gt_ptr, n, 20 + (exclude ? (size_t)W * 4 : 0),
                                    workspace_budget(), 28);
  PositionsArgs a{};
  a.X = c->emb[side];
  a.Y = c->emb[1];
  a.m = m;
  a.Dp = c->Dp;
  a.splits = scan_plan(c, 1, m, n, 0).splits;  // no list: one tile per split at least
  c->rec_splits = a.splits;
  a.row_ptr = exclude ? c->rp[side] : nullptr;
  a.col = exclude ? c->col[side] : nullptr;
  int32_t* d_gt = nullptr;
  rc = Carver::run(c, [&](Carver& cv) {
    const size_t ids = (size_t)ct.max_ids, nb = (size_t)ct.max_rows;
    d_gt = cv.take<int32_t>(ids);
    a.words = cv.take<unsigned long long>(ids);
    a.thr = cv.take<unsigned long long>(ids);
    a.counters = cv.take<uint32_t>(ids + nb);
    a.rank = cv.take<int32_t>(ids);
    a.g = cv.take<int32_t>(nb);
    a.bitmap = cv.take_if<uint32_t>(exclude, nb * (size_t)W);
    a.eligible = cv.take<int32_t>(nb);
    a.mrr = cv.take<float>(nb);
    a.auc = cv.take<float>(nb);
    // outside the per-row budget: per call
    a.maskw = cv.take<uint32_t>((size_t)W);
    a.gt_ptr = cv.take<int64_t>((size_t)n + 1);
    a.qrows = cv.take_if<int64_t>(rows != nullptr, (size_t)n);
  });
  if (rc) return rc;
  a.gt = d_gt;
  const std::vector<uint32_t> maskw = item_mask_words(m, item_mask);
  HIP_TRY(c, to_device(c, a.maskw, maskw.data(), maskw.size()));
  HIP_TRY(c, to_device(c, a.gt_ptr, gt_ptr, (size_t)n + 1));
  if (rows) HIP_TRY(c, to_device(c, a.qrows, rows, (size_t)n));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t b = 0; b + 1 < ct.cuts.size(); ++b) {  // one timed launch group per row batch
    a.r0 = ct.cuts[b];
    a.n = ct.cuts[b + 1] - ct.cuts[b];
    a.gt_base = gt_ptr[a.r0];
    const int64_t ids = gt_ptr[a.r0 + a.n] - a.gt_base;
    HIP_TRY(c, to_device(c, a.gt, gt_items + a.gt_base, (size_t)ids));
    ScopedTimer t(c, "rank_positions");
    HIP_TRY(c, launch_positions(a, c->stream));
    t.stop();
    if (rank) HIP_TRY(c, to_host(c, rank + a.gt_base, a.rank, (size_t)ids));
    if (eligible) HIP_TRY(c, to_host(c, eligible + a.r0, a.eligible, (size_t)a.n));
    if (mrr) HIP_TRY(c, to_host(c, mrr + a.r0, a.mrr, (size_t)a.n));
    if (auc) HIP_TRY(c, to_host(c, auc + a.r0, a.auc, (size_t)a.n));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  // scoring flops at the logical dim; bytes: the ground truth read, the ranks
  // and the three values per row written
  add_work(c, "rank_positions", 2.0 * (double)n * (double)m * (double)c->dim,
           (double)gt_ptr[n] * 4.0 + ((double)n + 1.0) * 8.0 + (double)gt_ptr[n] * 4.0 +
               (double)n * 12.0,
           n);
  return FRECSYS_OK;
}

int frecsys_csr_row_lengths(frecsys_ctx* c, int32_t side, const int64_t* rows, int64_t n_rows,
                            int64_t* lengths) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "csr_row_lengths: null context");
  const std::string w = "csr_row_lengths: ";
  if (side < 0 || side > 2) return fail(c, FRECSYS_ERR_INVALID, w + "bad side");
  if (n_rows < 0 || (n_rows > 0 && !lengths))
    return fail(c, FRECSYS_ERR_INVALID, w + "bad arguments");
  if (!c->rp[side]) return fail(c, FRECSYS_ERR_INVALID, w + "no CSR loaded on the side");
  const std::vector<int64_t>& hrp = side == 2 ? c->host_rp_eval : c->host_rp[side];
  const int64_t ns = (int64_t)hrp.size() - 1;
  if (!rows && n_rows > ns) return fail(c, FRECSYS_ERR_INVALID, w + "more rows than the side has");
  for (int64_t i = 0; i < n_rows; ++i) {
    const int64_t e = rows ? rows[i] : i;
    if (e < 0 || e >= ns)
      return fail(c, FRECSYS_ERR_INVALID, w + "row id " + std::to_string(e) + " out of range");
    lengths[i] = hrp[(size_t)e + 1] - hrp[(size_t)e];
  }
  return FRECSYS_OK;
}

int frecsys_explain(frecsys_ctx* c, int32_t side, const frecsys_solve_params* p,
                    const int64_t* rows, int64_t n_rows, const int64_t* tgt_ptr,
                    const int32_t* tgt_items, int32_t top, float* score, int32_t* top_items,
                    float* top_contrib, float* full) {
  if (!c) return fail(c, FRECSYS_ERR_INVALID, "explain: null context");
  const std::string w = "explain: ";
  int rc = check_query(c, w, side, FRECSYS_SIDE_EVAL, nullptr, 0, 0);
  if (rc) return rc;
  if (!p) return fail(c, FRECSYS_ERR_INVALID, w + "null params");
  if (p->kind != FRECSYS_KIND_IALS && p->kind != FRECSYS_KIND_WEIGHTED_U)
    return fail(c, FRECSYS_ERR_INVALID, w + "kind must be IALS or WEIGHTED_U");
  if (top < 1 || top > kExplainMaxTop)
    return fail(c, FRECSYS_ERR_INVALID,
                w + "top must be in [1, " + std::to_string(kExplainMaxTop) + "]");
  if (c->dim > 256)
    return fail(c, FRECSYS_ERR_UNSUPPORTED,
                w + "explanations are built for dim <= 256 (dim " + std::to_string(c->dim) + ")");
  if (n_rows < 0) return fail(c, FRECSYS_ERR_INVALID, w + "negative row count");
  if (n_rows == 0) return FRECSYS_OK;
  if (!tgt_ptr) return fail(c, FRECSYS_ERR_INVALID, w + "null pointer");
  if (!c->rp[side]) return fail(c, FRECSYS_ERR_INVALID, w + "no CSR loaded on the side");
  const int64_t m = c->n[1], n = n_rows;
  if ((rc = check_rows(c, w, side, FRECSYS_SIDE_ITEM, false, rows, n))) return rc;
  if ((rc = check_candidates(c, w, tgt_ptr, tgt_items, n, m))) return rc;
  const int64_t pairs = tgt_ptr[n];
  if (pairs == 0) return FRECSYS_OK;
  if (!score || !top_items || !top_contrib)
    return fail(c, FRECSYS_ERR_INVALID, w + "null pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  const std::vector<int64_t>& hrp = side == 2 ? c->host_rp_eval : c->host_rp[side];
  auto hist = [&](int64_t i) {
    const int64_t e = rows ? rows[i] : i;
    return hrp[(size_t)e + 1] - hrp[(size_t)e];
  };
  // Rows cut in the manner of cut_by_candidates, by the contributions (h per
  // pair) and the per-pair outputs of a batch; at least one row each.
  const size_t per_pair = 4 + (size_t)top * 8 + 4 + 4, budget = workspace_budget();
  std::vector<int64_t> cuts{0};
  int64_t max_rows = 0, max_pairs = 0, max_contrib = 0;
  for (int64_t r0 = 0; r0 < n;) {
    size_t bytes = 0;
    int64_t r1 = r0, contrib = 0;
    while (r1 < n) {
      const int64_t mt = tgt_ptr[r1 + 1] - tgt_ptr[r1];
      const size_t add = 8 + (size_t)mt * per_pair + (size_t)mt * (size_t)hist(r1) * 4;
      if (r1 > r0 && bytes + add > budget) break;
      bytes += add;
      contrib += mt * hist(r1);
      ++r1;
    }
    max_rows = std::max(max_rows, r1 - r0);
    max_pairs = std::max(max_pairs, tgt_ptr[r1] - tgt_ptr[r0]);
    max_contrib = std::max(max_contrib, contrib);
    cuts.push_back(r1);
    r0 = r1;
  }
  int dev_cus = 256;
  (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c->device);
  const int grid = (int)std::min<int64_t>(max_rows, 4 * (int64_t)dev_cus);
  const bool ukind = p->kind == FRECSYS_KIND_WEIGHTED_U;
  ExplainArgs a{};
  a.kind = p->kind;
  a.Dp = c->Dp;
  a.row_ptr = c->rp[side];
  a.col = c->col[side];
  a.X = c->emb[1];
  a.n_other = m;
  a.G = c->gram[1];
  a.reg = p->reg;
  a.reg_exp = p->reg_exp;
  a.w = p->unobserved_weight;
  a.lambda_is_reg = p->lambda_is_reg;
  a.fail = c->d_fail;
  a.top = top;
  int32_t *d_prow = nullptr, *d_tgt = nullptr, *d_order = nullptr;
  int64_t* d_coff = nullptr;
  float* d_weight = nullptr;
  rc = Carver::run(c, [&](Carver& cv) {
    a.contrib = cv.take<float>((size_t)max_contrib);
    a.score = cv.take<float>((size_t)max_pairs);
    a.top_items = cv.take<int32_t>((size_t)max_pairs * top);
    a.top_contrib = cv.take<float>((size_t)max_pairs * top);
    d_prow = cv.take<int32_t>((size_t)max_pairs);
    d_tgt = cv.take<int32_t>((size_t)max_pairs);
    d_coff = cv.take<int64_t>((size_t)max_rows);
    d_order = cv.take<int32_t>((size_t)max_rows);
    a.wws = cv.take<float>((size_t)grid * kExplainGroup * explain_ld(c->Dp));
    a.tgt_ptr = cv.take<int64_t>((size_t)n + 1);
    a.qrows = cv.take_if<int64_t>(rows != nullptr, (size_t)n);
    d_weight = cv.take_if<float>(ukind && p->entity_weight, (size_t)c->n[side]);
  });
  if (rc) return rc;
  a.prow = d_prow;
  a.tgt = d_tgt;
  a.coff = d_coff;
  a.order = d_order;
  a.entity_weight = d_weight;
  HIP_TRY(c, to_device(c, a.tgt_ptr, tgt_ptr, (size_t)n + 1));
  if (rows) HIP_TRY(c, to_device(c, a.qrows, rows, (size_t)n));
  if (d_weight) HIP_TRY(c, to_device(c, a.entity_weight, p->entity_weight, (size_t)c->n[side]));
  HIP_TRY(c, hipMemsetAsync(c->d_fail, 0xFF, sizeof(unsigned long long), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<int32_t> prow, order;
  std::vector<int64_t> coff, cost;
  int64_t full_at = 0;
  double flops = 0.0, bytes = 0.0;
  const double d = c->dim;
  for (size_t b = 0; b + 1 < cuts.size(); ++b) {  // one timed launch group per row batch
    a.r0 = cuts[b];
    a.n = cuts[b + 1] - cuts[b];
    a.tgt_base = tgt_ptr[a.r0];
    const int64_t np = tgt_ptr[a.r0 + a.n] - a.tgt_base;
    if (np == 0) continue;
    prow.clear();
    coff.assign((size_t)a.n, 0);
    cost.assign((size_t)a.n, 0);
    order.resize((size_t)a.n);
    int64_t contrib = 0;
    for (int64_t i = 0; i < a.n; ++i) {
      const int64_t mt = tgt_ptr[a.r0 + i + 1] - tgt_ptr[a.r0 + i], h = hist(a.r0 + i);
      coff[(size_t)i] = contrib;
      contrib += mt * h;
      prow.insert(prow.end(), (size_t)mt, (int32_t)i);
      order[(size_t)i] = (int32_t)i;
      // history rows streamed: once to assemble, once per group of targets
      cost[(size_t)i] = mt > 0 ? h * (1 + (mt + kExplainGroup - 1) / kExplainGroup) : 0;
      if (mt > 0 && h > 0) {
        const double groups = (double)((mt + kExplainGroup - 1) / kExplainGroup);
        flops += (double)h * d * d + d * d * d / 3.0 + 2.0 * d * d * (double)mt +
                 2.0 * (double)h * d * (double)mt;
        bytes += (1.0 + groups) * (double)h * (d * 4.0 + 4.0) + (double)mt * d * 4.0;
      }
    }
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t x, int32_t y) { return cost[(size_t)x] > cost[(size_t)y]; });
    HIP_TRY(c, to_device(c, a.order, order.data(), order.size()));
    HIP_TRY(c, to_device(c, a.prow, prow.data(), prow.size()));
    HIP_TRY(c, to_device(c, a.coff, coff.data(), coff.size()));
    HIP_TRY(c, to_device(c, a.tgt, tgt_items + a.tgt_base, (size_t)np));
    ScopedTimer t(c, "explain");
    HIP_TRY(c, launch_explain(a, (int)std::min<int64_t>(a.n, grid), c->stream));
    HIP_TRY(c, launch_explain_select(a, np, c->stream));
    t.stop();
    HIP_TRY(c, to_host(c, score + a.tgt_base, a.score, (size_t)np));
    HIP_TRY(c, to_host(c, top_items + a.tgt_base * top, a.top_items, (size_t)np * top));
    HIP_TRY(c, to_host(c, top_contrib + a.tgt_base * top, a.top_contrib, (size_t)np * top));
    if (full && contrib > 0) HIP_TRY(c, to_host(c, full + full_at, a.contrib, (size_t)contrib));
    full_at += contrib;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  unsigned long long f = ~0ull;
  HIP_TRY(c, hipMemcpy(&f, c->d_fail, sizeof(f), hipMemcpyDeviceToHost));
  add_work(c, "explain", flops, bytes, n);
  if (f != ~0ull) {
    c->err_entity = (int64_t)f - 1;
    return fail(c, FRECSYS_ERR_NOT_SPD, w + "LLT failed (matrix not SPD) for entity " +
                                            std::to_string(c->err_entity));
  }
  return FRECSYS_OK;
}

}  // extern "C"
