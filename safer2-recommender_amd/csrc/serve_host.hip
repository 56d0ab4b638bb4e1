// serve_host.hip -- the context-free host arithmetic of the C-ABI
// (include/frecsys_hip.h): frecsys_sample_negatives, frecsys_list_metrics,
// frecsys_position_metrics, frecsys_metric_cvar, frecsys_mmr_select,
// frecsys_dpp_select, frecsys_list_quality, frecsys_exposure_summary -- what
// the device calls of serve.hip compute, restated on the host for the model
// layer and the tests -- and the one definition of what serve.h declares.  No
// HIP runtime call and no context: errors go to fail(nullptr, ...).
//
// Floating point.  The library's flags let the compiler contract, and the
// double arithmetic of frecsys_list_quality is compiled so.  The two
// selections restate device kernels to the bit: they and every helper lifted
// out of them carry `#pragma clang fp contract(off)`, per function.
#include <atomic>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <thread>

#include "../include/frecsys/parallel.h"
#include "serve.h"

namespace frecsys_hip {

int check_diversify(frecsys_ctx* c, const std::string& w, int32_t k, int32_t pool, float lam,
                    int32_t flags, int32_t known_flags) {
  if (pool < 1 || pool > kDiversifyMaxPool)
    return fail(c, FRECSYS_ERR_INVALID, w + "pool must be in [1, 1024]");
  if (k < 1 || k > pool) return fail(c, FRECSYS_ERR_INVALID, w + "k must be in [1, pool]");
  if (!(lam >= 0.0f && lam <= 1.0f))
    return fail(c, FRECSYS_ERR_INVALID, w + "lam must be in [0, 1]");
  if (flags & ~known_flags) return fail(c, FRECSYS_ERR_INVALID, w + "unknown flag");
  return FRECSYS_OK;
}

int check_dpp(frecsys_ctx* c, const std::string& w, int32_t k, int32_t pool, float theta, float eps,
              int32_t flags, int32_t known_flags) {
  if (int rc = check_diversify(c, w, k, pool, 0.0f, flags, known_flags)) return rc;
  if (!(theta >= 0.0f && std::isfinite(theta)))
    return fail(c, FRECSYS_ERR_INVALID, w + "theta must be finite and >= 0");
  if (!(eps > 0.0f && eps <= 1.0f)) return fail(c, FRECSYS_ERR_INVALID, w + "eps must be in (0, 1]");
  return FRECSYS_OK;
}

std::string pool_error(const int32_t* lists, const float* list_scores, int64_t n, int32_t pool,
                       int64_t m, bool raw) {
  for (int64_t i = 0; i < n; ++i) {
    float smax = -INFINITY, smin = INFINITY;
    bool any = false;
    for (int32_t b = 0; b < pool; ++b) {
      const int32_t id = lists[i * pool + b];
      if (id < 0) continue;
      if (id >= m) return "item id " + std::to_string(id) + " out of range";
      const float s = list_scores[i * pool + b];
      if (!std::isfinite(s)) return "non-finite score in row " + std::to_string(i);
      smax = std::fmax(smax, s);
      smin = std::fmin(smin, s);
      any = true;
    }
    if (any && !raw && !std::isfinite(smax - smin))
      return "score range of row " + std::to_string(i) + " is not finite";
  }
  return "";
}

std::string quality_args_error(const QualityRequest& q, int32_t max_k, int64_t n_items,
                               bool others) {
  if (!q.k_list || q.nk < 1 || q.nk > kMetricMaxCutoffs)
    return "k_list must hold 1 to " + std::to_string(kMetricMaxCutoffs) + " cut-offs";
  for (int32_t i = 0; i < q.nk; ++i)
    if (q.k_list[i] < 1 || q.k_list[i] > max_k)
      return "cut-offs must be in [1, " + std::to_string(max_k) + "]";
  if (!q.ild && !q.novelty && !q.exposure && !others) return "every output is null";
  if (q.novelty && !q.item_weight) return "novelty needs item_weight";
  if (q.item_weight && !q.novelty) return "item_weight without a novelty output";
  if (q.item_weight)
    for (int64_t j = 0; j < n_items; ++j)
      if (!std::isfinite(q.item_weight[j]))
        return "item_weight[" + std::to_string(j) + "] is not finite";
  return "";
}

std::string lists_error(const int32_t* lists, int64_t n, int32_t list_k, int64_t m) {
  if (n < 0) return "negative row count";
  if (n > 0 && !lists) return "null lists";
  if (n > INT64_MAX / list_k) return "n * list_k overflows";
  for (int64_t p = 0; p < n * list_k; ++p)
    if (lists[p] >= m) return "item id " + std::to_string(lists[p]) + " out of range";
  return "";
}

const MetricTables& metric_tables() {
  static const MetricTables tab = [] {
    MetricTables t;
    t.idcg[0] = 0.0;
    for (int j = 0; j < kMetricMaxK; ++j) {
      t.gain[j] = 1.0 / std::log2(j + 2.0);
      t.idcg[j + 1] = t.idcg[j] + t.gain[j];
    }
    return t;
  }();
  return tab;
}

// The rules of a ground-truth pointer array over n rows: starts at 0, monotone,
// no empty row; "" when fine.
static std::string gt_ptr_error(int64_t n, const int64_t* gt_ptr) {
  if (gt_ptr[0] != 0) return "gt_ptr[0] must be 0";
  for (int64_t i = 0; i < n; ++i) {
    if (gt_ptr[i + 1] < gt_ptr[i]) return "gt_ptr not monotone at row " + std::to_string(i);
    if (gt_ptr[i + 1] == gt_ptr[i]) return "row " + std::to_string(i) + " has no ground truth";
  }
  return "";
}

std::string metric_args_error(int64_t n, const int64_t* gt_ptr, const int32_t* gt_items,
                              const int32_t* k_list, int32_t nk, int64_t n_items,
                              int32_t* max_k) {
  if (n < 0 || !gt_ptr || !k_list) return "bad arguments (null gt_ptr / k_list, n < 0)";
  if (nk < 1 || nk > kMetricMaxCutoffs)
    return "nk must be in [1, " + std::to_string(kMetricMaxCutoffs) + "]";
  int32_t mk = 0;
  for (int32_t q = 0; q < nk; ++q) {
    if (k_list[q] < 1 || k_list[q] > kMetricMaxK)
      return "k_list[" + std::to_string(q) + "] must be in [1, " + std::to_string(kMetricMaxK) +
             "]";
    mk = std::max(mk, k_list[q]);
  }
  *max_k = mk;
  const std::string e = gt_ptr_error(n, gt_ptr);
  if (!e.empty()) return e;
  if (n > 0 && !gt_items) return "null gt_items";
  for (int64_t p = 0; p < gt_ptr[n]; ++p)
    if (gt_items[p] < 0 || (n_items >= 0 && gt_items[p] >= n_items))
      return "ground-truth id " + std::to_string(gt_items[p]) + " out of range";
  return "";
}

void sorted_ground_truth(int64_t n, const int64_t* gt_ptr, const int32_t* gt_items,
                         std::vector<int64_t>* sp, std::vector<int32_t>* sg) {
  const int64_t total = gt_ptr[n];
  sg->assign(gt_items, gt_items + total);
  sp->assign((size_t)n + 1, 0);
  std::vector<int64_t> cnt((size_t)n);
  int32_t* base = sg->data();
  auto work = [&](int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) {
      int32_t* p = base + gt_ptr[i];
      int32_t* e = base + gt_ptr[i + 1];
      bool ascending = true;
      for (int32_t* q = p + 1; q < e; ++q)
        if (q[-1] >= q[0]) {
          ascending = false;
          break;
        }
      if (!ascending) {
        std::sort(p, e);
        e = std::unique(p, e);
      }
      cnt[(size_t)i] = e - p;
    }
  };
  const int nt = total < (1 << 16)
                     ? 1
                     : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (nt == 1) {
    work(0, n);
  } else {
    std::vector<int64_t> bounds((size_t)nt + 1);
    partition_rows(n, gt_ptr, nt, bounds.data());
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work, bounds[(size_t)t], bounds[(size_t)t + 1]);
    for (auto& t : th) t.join();
  }
  int64_t w = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (w != gt_ptr[i]) std::memmove(base + w, base + gt_ptr[i], sizeof(int32_t) * (size_t)cnt[(size_t)i]);
    w += cnt[(size_t)i];
    (*sp)[(size_t)i + 1] = w;
  }
  sg->resize((size_t)w);
}

}  // namespace frecsys_hip

namespace {

// splitmix64's finaliser and its increment: the generator of the sampled
// negatives (include/frecsys_hip.h), uint64 arithmetic that wraps.
inline uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// What frecsys_mmr_select and frecsys_dpp_select share beside their own
// selection loops and cost formulas.

// The product of two item rows: acc = fmaf(x[c], y[c], acc), c ascending from +0.
struct Dot {
  const float* table;
  int64_t ld;
  int32_t dim;
  float operator()(int32_t x, int32_t y) const {
#pragma clang fp contract(off)
    const float* px = table + (int64_t)x * ld;
    const float* py = table + (int64_t)y * ld;
    float acc = 0.0f;
    for (int32_t cc = 0; cc < dim; ++cc) acc = std::fmaf(px[cc], py[cc], acc);
    return acc;
  }
};

// The argument checks behind check_diversify / check_dpp.  n == 0 passes: the
// caller returns then.
int check_select(const std::string& w, const float* item_table, int64_t n_items, int32_t dim,
                 int64_t ld, const int32_t* lists, const float* list_scores, int64_t n,
                 int32_t pool, bool raw, const int32_t* items, const float* scores) {
  if (n < 0) return fail(nullptr, FRECSYS_ERR_INVALID, w + "negative row count");
  if (n == 0) return FRECSYS_OK;
  if (!item_table || n_items < 1 || dim < 1 || ld < dim)
    return fail(nullptr, FRECSYS_ERR_INVALID, w + "bad item table (null, n_items < 1, ld < dim)");
  if (!lists || !list_scores || !items || !scores)
    return fail(nullptr, FRECSYS_ERR_INVALID, w + "null pointer");
  const std::string e = pool_error(lists, list_scores, n, pool, n_items, raw);
  if (!e.empty()) return fail(nullptr, FRECSYS_ERR_INVALID, w + e);
  return FRECSYS_OK;
}

// One pool: which slots are filled (returns their count), per filled slot the
// inverse norm of its item row (0 for a zero row; nz, unless null: 1 / 0) and
// its relevance: the score, or normalised (score - min) / (max - min), 0 at range 0.
int32_t pool_row(const Dot& dot, const int32_t* ids, const float* sc, int32_t pool, bool raw,
                 uint8_t* alive, float* inv, float* rel, float* nz) {
#pragma clang fp contract(off)
  float smax = -INFINITY, smin = INFINITY;
  int32_t p = 0;
  for (int32_t b = 0; b < pool; ++b) {
    alive[b] = ids[b] >= 0;
    if (!alive[b]) continue;
    ++p;
    smax = std::fmax(smax, sc[b]);
    smin = std::fmin(smin, sc[b]);
    const float n2 = dot(ids[b], ids[b]);
    inv[b] = n2 > 0.0f ? 1.0f / std::sqrt(n2) : 0.0f;
    if (nz) nz[b] = n2 > 0.0f ? 1.0f : 0.0f;
  }
  const float range = smax - smin;
  for (int32_t b = 0; b < pool; ++b)
    if (alive[b]) rel[b] = raw ? sc[b] : (range > 0.0f ? (sc[b] - smin) / range : 0.0f);
  return p;
}

// The argmax word of a step: the value's order-preserving key (rerank.hip's)
// above the slot complemented: the largest word is the largest value at its
// lowest slot.
inline uint32_t score_key(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float score_unkey(uint32_t key) {
  const uint32_t u = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  float v;
  std::memcpy(&v, &u, 4);
  return v;
}
inline uint64_t slot_word(uint32_t key, int32_t b) {
  return ((uint64_t)key << 32) | (0xFFFFFFFFu - (uint32_t)b);
}
inline int32_t word_slot(uint64_t word) { return (int32_t)(0xFFFFFFFFu - (uint32_t)word); }

// Slots [steps, k) of row i: beyond the filled count.
void fill_tail(int64_t i, int32_t steps, int32_t k, int32_t* items, float* scores, float* extra) {
  for (int32_t t = steps; t < k; ++t) {
    items[i * k + t] = -1;
    scores[i * k + t] = -FLT_MAX;
    if (extra) extra[i * k + t] = -FLT_MAX;
  }
}

// Rows are independent: host threads over row ranges when there is enough work.
template <typename Work>
void for_rows(int64_t n, double cost, Work work) {
  const int nt = cost < 1e8 ? 1
                            : (int)std::min<int64_t>(
                                  n, std::min(16u, std::max(1u, std::thread::hardware_concurrency())));
  if (nt <= 1) {
    work(0, n);
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work, n * t / nt, n * (t + 1) / nt);
    for (auto& t : th) t.join();
  }
}

}  // namespace

extern "C" {

int frecsys_mmr_select(const float* item_table, int64_t n_items, int32_t dim, int64_t ld,
                       const int32_t* lists, const float* list_scores, int64_t n, int32_t pool,
                       int32_t k, float lam, int32_t flags, int32_t* items, float* scores,
                       float* mmr) {
#pragma clang fp contract(off)
  const std::string w = "mmr_select: ";
  int rc = check_diversify(nullptr, w, k, pool, lam, flags, FRECSYS_DIV_RAW_SCORES);
  if (rc) return rc;
  const bool raw = (flags & FRECSYS_DIV_RAW_SCORES) != 0;
  rc = check_select(w, item_table, n_items, dim, ld, lists, list_scores, n, pool, raw, items,
                    scores);
  if (rc || n == 0) return rc;
  const float oml = 1.0f - lam;
  const Dot dot{item_table, ld, dim};
  auto work = [&](int64_t i0, int64_t i1) {
    std::vector<float> base((size_t)pool), mm((size_t)pool), inv((size_t)pool);
    std::vector<uint8_t> alive((size_t)pool);
    for (int64_t i = i0; i < i1; ++i) {
      const int32_t* ids = lists + i * pool;
      const float* sc = list_scores + i * pool;
      const int32_t p =
          pool_row(dot, ids, sc, pool, raw, alive.data(), inv.data(), base.data(), nullptr);
      for (int32_t b = 0; b < pool; ++b) {
        if (!alive[(size_t)b]) continue;
        base[(size_t)b] = lam * base[(size_t)b];
        mm[(size_t)b] = -INFINITY;
      }
      const int32_t steps = std::min(p, k);
      for (int32_t t = 0; t < steps; ++t) {
        uint64_t best = 0;
        for (int32_t b = 0; b < pool; ++b) {
          if (!alive[(size_t)b]) continue;
          float v;
          if (t == 0) {
            v = base[(size_t)b] + 0.0f;
          } else {
            const float pen = oml * mm[(size_t)b];
            v = (base[(size_t)b] - pen) + 0.0f;
          }
          best = std::max(best, slot_word(score_key(v), b));
        }
        const int32_t s = word_slot(best);
        items[i * k + t] = ids[s];
        scores[i * k + t] = sc[s];
        if (mmr) mmr[i * k + t] = score_unkey((uint32_t)(best >> 32));
        alive[(size_t)s] = 0;
        if (t + 1 == steps) break;
        for (int32_t b = 0; b < pool; ++b) {
          if (!alive[(size_t)b]) continue;
          const float g = dot(ids[s], ids[b]);
          const float gs = g * inv[(size_t)s];
          const float cs = gs * inv[(size_t)b] + 0.0f;
          mm[(size_t)b] = std::fmax(mm[(size_t)b], cs);
        }
      }
      fill_tail(i, steps, k, items, scores, mmr);
    }
  };
  for_rows(n, (double)n * pool * (double)k * dim, work);
  return FRECSYS_OK;
}

int frecsys_dpp_select(const float* item_table, int64_t n_items, int32_t dim, int64_t ld,
                       const int32_t* lists, const float* list_scores, int64_t n, int32_t pool,
                       int32_t k, float theta, float eps, int32_t flags, int32_t* items,
                       float* scores, float* gain) {
#pragma clang fp contract(off)
  const std::string w = "dpp_select: ";
  int rc = check_dpp(nullptr, w, k, pool, theta, eps, flags, FRECSYS_DIV_RAW_SCORES);
  if (rc) return rc;
  const bool raw = (flags & FRECSYS_DIV_RAW_SCORES) != 0;
  rc = check_select(w, item_table, n_items, dim, ld, lists, list_scores, n, pool, raw, items,
                    scores);
  if (rc || n == 0) return rc;
  const Dot dot{item_table, ld, dim};
  auto work = [&](int64_t i0, int64_t i1) {
    const size_t P = (size_t)pool;
    std::vector<float> wq(P), r(P), inv(P), C((size_t)k * P);
    std::vector<uint8_t> alive(P);
    for (int64_t i = i0; i < i1; ++i) {
      const int32_t* ids = lists + i * pool;
      const float* sc = list_scores + i * pool;
      const int32_t p =
          pool_row(dot, ids, sc, pool, raw, alive.data(), inv.data(), wq.data(), r.data());
      for (int32_t b = 0; b < pool; ++b) {
        if (!alive[(size_t)b]) continue;
        const float x = theta * wq[(size_t)b];
        wq[(size_t)b] = dpp_exp2(std::fmin(std::fmax(x, -64.0f), 64.0f));
      }
      const int32_t steps = std::min(p, k);
      int32_t m = 0;
      for (int32_t t = 0; t < steps; ++t) {
        uint64_t best = 0;
        for (int32_t b = 0; b < pool; ++b) {
          if (!alive[(size_t)b]) continue;
          uint32_t key = 0;  // below eps: the fallback's word, the lowest slot wins
          if (r[(size_t)b] >= eps) key = score_key(wq[(size_t)b] * r[(size_t)b] + 0.0f);
          best = std::max(best, slot_word(key, b));
        }
        const int32_t s = word_slot(best);
        const uint32_t key = (uint32_t)(best >> 32);
        items[i * k + t] = ids[s];
        scores[i * k + t] = sc[s];
        if (gain) gain[i * k + t] = key ? score_unkey(key) : 0.0f;
        alive[(size_t)s] = 0;
        if (key == 0 || t + 1 == steps) continue;  // the last step's update is never read
        const float delta = std::sqrt(r[(size_t)s]);
        const float* cs = C.data() + (size_t)s;
        for (int32_t b = 0; b < pool; ++b) {
          if (!alive[(size_t)b]) continue;
          const float g = dot(ids[s], ids[b]);
          const float gs = g * inv[(size_t)s];
          const float sim = gs * inv[(size_t)b] + 0.0f;
          float acc = 0.0f;
          for (int32_t uu = 0; uu < m; ++uu)
            acc = std::fmaf(C[(size_t)uu * P + (size_t)b], cs[(size_t)uu * P], acc);
          const float d = sim - acc;
          const float ev = d / delta;
          C[(size_t)m * P + (size_t)b] = ev;
          r[(size_t)b] = std::fmaf(-ev, ev, r[(size_t)b]);
        }
        ++m;
      }
      fill_tail(i, steps, k, items, scores, gain);
    }
  };
  for_rows(n, (double)n * pool * (double)k * ((double)dim + 0.5 * k), work);
  return FRECSYS_OK;
}

int frecsys_list_quality(const float* item_table, int64_t n_items, int32_t dim, int64_t ld,
                         const int32_t* lists, int64_t n, int32_t list_k, const int32_t* k_list,
                         int32_t nk, const float* item_weight, float* ild, float* novelty,
                         int64_t* exposure) {
  const std::string w = "list_quality: ";
  if (list_k < 1) return fail(nullptr, FRECSYS_ERR_INVALID, w + "list_k must be positive");
  if (n_items < 1) return fail(nullptr, FRECSYS_ERR_INVALID, w + "n_items must be positive");
  const QualityRequest ql{k_list, nk, item_weight, ild, novelty, exposure};
  std::string e = quality_args_error(ql, std::min<int32_t>(kMetricMaxK, list_k), n_items, false);
  if (!e.empty()) return fail(nullptr, FRECSYS_ERR_INVALID, w + e);
  if (ild && (!item_table || dim < 1 || ld < dim))
    return fail(nullptr, FRECSYS_ERR_INVALID, w + "bad item table (null, dim < 1, ld < dim)");
  e = lists_error(lists, n, list_k, n_items);
  if (!e.empty()) return fail(nullptr, FRECSYS_ERR_INVALID, w + e);
  if (exposure) std::memset(exposure, 0, sizeof(int64_t) * (size_t)nk * (size_t)n_items);
  const int32_t mk = max_cutoff(k_list, nk);
  // C and the weight sum after every filled slot count 0 .. mk, then per cut-off
  std::vector<double> s(ild ? (size_t)dim : 0), run_c((size_t)mk + 1), run_w((size_t)mk + 1);
  std::vector<int32_t> filled_below((size_t)mk + 1);  // filled slots among positions < j
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* list = lists + i * list_k;
    std::fill(s.begin(), s.end(), 0.0);
    double C = 0.0, W = 0.0;
    int32_t b = 0;
    run_c[0] = run_w[0] = 0.0;
    for (int32_t j = 0; j < mk; ++j) {
      filled_below[(size_t)j] = b;
      const int32_t id = list[j];
      if (id < 0) continue;
      if (ild) {
        const float* y = item_table + (int64_t)id * ld;
        double n2 = 0.0, ys = 0.0;
        for (int32_t cc = 0; cc < dim; ++cc) n2 += (double)y[cc] * (double)y[cc];
        const double inv = n2 > 0.0 ? 1.0 / std::sqrt(n2) : 0.0;
        for (int32_t cc = 0; cc < dim; ++cc) ys += (inv * (double)y[cc]) * s[(size_t)cc];
        C += ys;
        for (int32_t cc = 0; cc < dim; ++cc) s[(size_t)cc] += inv * (double)y[cc];
      }
      if (item_weight) W += (double)item_weight[id];
      if (exposure)
        for (int32_t q = 0; q < nk; ++q)
          if (j < k_list[q]) ++exposure[(int64_t)q * n_items + id];
      ++b;
      run_c[(size_t)b] = C;
      run_w[(size_t)b] = W;
    }
    filled_below[(size_t)mk] = b;
    for (int32_t q = 0; q < nk; ++q) {
      const int32_t nq = filled_below[(size_t)k_list[q]];
      if (ild)
        ild[i * nk + q] =
            nq >= 2 ? (float)(1.0 - run_c[(size_t)nq] / (double)((int64_t)nq * (nq - 1) / 2))
                    : 0.0f;
      if (novelty) novelty[i * nk + q] = nq >= 1 ? (float)(run_w[(size_t)nq] / (double)nq) : 0.0f;
    }
  }
  return FRECSYS_OK;
}

int frecsys_exposure_summary(const int64_t* exposure, int64_t n_items, const uint8_t* item_mask,
                             double* coverage, double* gini, int64_t* total, int64_t* covered) {
  const std::string w = "exposure_summary: ";
  if (!exposure || n_items < 1)
    return fail(nullptr, FRECSYS_ERR_INVALID, w + "bad arguments (null exposure, n_items < 1)");
  std::vector<int64_t> cs;
  int64_t S = 0, cov = 0;
  for (int64_t j = 0; j < n_items; ++j) {
    if (item_mask && !item_mask[j]) continue;
    if (exposure[j] < 0) return fail(nullptr, FRECSYS_ERR_INVALID, w + "negative count");
    if (exposure[j] > INT64_MAX - S) return fail(nullptr, FRECSYS_ERR_INVALID, w + "counts overflow");
    cs.push_back(exposure[j]);
    S += exposure[j];
    cov += exposure[j] > 0;
  }
  const int64_t M = (int64_t)cs.size();
  double cv = 0.0, g = 0.0;
  if (M > 0 && S > 0) {
    std::sort(cs.begin(), cs.end());
    __int128 num = 0;  // sum over the ascending counts of (2 i - M - 1) c_(i), i = 1 .. M
    for (int64_t i = 0; i < M; ++i) num += (__int128)(2 * (i + 1) - M - 1) * cs[(size_t)i];
    cv = (double)cov / (double)M;
    g = (double)num / (double)((__int128)M * S);
  }
  if (coverage) *coverage = cv;
  if (gini) *gini = g;
  if (total) *total = S;
  if (covered) *covered = cov;
  return FRECSYS_OK;
}

int frecsys_sample_negatives(int64_t n_items, const uint8_t* item_mask, const int64_t* row_ids,
                             int64_t n_rows, const int64_t* hist_ptr, const int32_t* hist_items,
                             const int64_t* gt_ptr, const int32_t* gt_items, int32_t n_neg,
                             uint64_t seed, int32_t* neg_count, int32_t* negatives) {
  const std::string w = "sample_negatives: ";
  if (n_items < 1 || n_items > INT32_MAX)
    return fail(nullptr, FRECSYS_ERR_INVALID, w + "n_items must be in [1, 2^31)");
  if (n_rows < 0) return fail(nullptr, FRECSYS_ERR_INVALID, w + "negative row count");
  if (n_neg < 0) return fail(nullptr, FRECSYS_ERR_INVALID, w + "n_neg must not be negative");
  if (n_neg > 0 && n_rows > INT64_MAX / n_neg)
    return fail(nullptr, FRECSYS_ERR_INVALID, w + "n_rows * n_neg overflows");
  if (n_rows == 0) return FRECSYS_OK;
  if (!neg_count) return fail(nullptr, FRECSYS_ERR_INVALID, w + "null neg_count");
  const int64_t n = n_rows, m = n_items;
  if (row_ids)
    for (int64_t i = 0; i < n; ++i)
      if (row_ids[i] < 0)
        return fail(nullptr, FRECSYS_ERR_INVALID,
                    w + "row id " + std::to_string(row_ids[i]) + " out of range");
  if (!hist_ptr && hist_items)
    return fail(nullptr, FRECSYS_ERR_INVALID, w + "hist_items without hist_ptr");
  if (hist_ptr) {
    if (hist_ptr[0] < 0) return fail(nullptr, FRECSYS_ERR_INVALID, w + "negative hist_ptr");
    for (int64_t i = 0; i < n; ++i)
      if (hist_ptr[i + 1] < hist_ptr[i])
        return fail(nullptr, FRECSYS_ERR_INVALID,
                    w + "hist_ptr not monotone at row " + std::to_string(i));
    if (hist_ptr[n] > hist_ptr[0] && !hist_items)
      return fail(nullptr, FRECSYS_ERR_INVALID, w + "null hist_items");
  }
  {
    const int32_t one = 1;
    int32_t mk = 0;
    const std::string e = metric_args_error(n, gt_ptr, gt_items, &one, 1, m, &mk);
    if (!e.empty()) return fail(nullptr, FRECSYS_ERR_INVALID, w + e);
  }
  std::vector<int32_t> dlist;
  int64_t M = m;
  if (item_mask) {
    for (int64_t j = 0; j < m; ++j)
      if (item_mask[j]) dlist.push_back((int32_t)j);
    M = (int64_t)dlist.size();
  }
  const uint64_t cap = kSampleCapBase + kSampleCapPerNeg * (uint64_t)n_neg;
  std::atomic<int64_t> capped{-1};
  // rows on the host thread pool; a task keeps one bitmap of the items and
  // clears the bits of a row after it (blocked = history and ground truth,
  // then the taken ids)
  frecsys::ThreadPool::Get().ParallelFor(n, 64, [&](int64_t lo, int64_t hi) {
    std::vector<uint64_t> bm((size_t)((m + 63) / 64), 0ull);
    std::vector<int32_t> set;  // ids whose bit this row set
    auto mark = [&](int64_t j) {
      uint64_t& wd = bm[(size_t)(j >> 6)];
      const uint64_t b = 1ull << (j & 63);
      if (wd & b) return false;
      wd |= b;
      set.push_back((int32_t)j);
      return true;
    };
    for (int64_t i = lo; i < hi; ++i) {
      set.clear();
      int64_t blocked = 0;  // distinct blocked ids that lie in D
      if (hist_ptr)
        for (int64_t p = hist_ptr[i]; p < hist_ptr[i + 1]; ++p) {
          const int64_t j = hist_items[p];
          if (j >= 0 && j < m && mark(j) && (!item_mask || item_mask[j])) ++blocked;
        }
      for (int64_t p = gt_ptr[i]; p < gt_ptr[i + 1]; ++p) {
        const int64_t j = gt_items[p];
        if (mark(j) && (!item_mask || item_mask[j])) ++blocked;
      }
      const int64_t E = M - blocked;
      int32_t* out = negatives ? negatives + i * n_neg : nullptr;
      if (whole_pool_row(n_neg, E, M)) {
        neg_count[i] = (int32_t)E;
        if (out) std::fill(out, out + n_neg, -1);
      } else {
        neg_count[i] = n_neg;
        const uint64_t r = (uint64_t)(row_ids ? row_ids[i] : i);
        const uint64_t key = mix64(seed + kGolden * (r + 1));
        int32_t have = 0;
        for (uint64_t t = 0; have < n_neg; ++t) {
          if (t >= cap) {
            int64_t none = -1;
            capped.compare_exchange_strong(none, i);
            break;
          }
          const uint64_t x = mix64(key + kGolden * (t + 1));
          const uint64_t idx = ((x >> 32) * (uint64_t)M) >> 32;
          const int64_t j = item_mask ? dlist[(size_t)idx] : (int64_t)idx;
          if (!mark(j)) continue;
          if (out) out[have] = (int32_t)j;
          ++have;
        }
      }
      for (const int32_t j : set) bm[(size_t)(j >> 6)] &= ~(1ull << (j & 63));
    }
  });
  if (capped.load() >= 0)
    return fail(nullptr, FRECSYS_ERR_HIP,
                w + "the draws of query row " + std::to_string(capped.load()) +
                    " reached the cap");
  return FRECSYS_OK;
}

int frecsys_list_metrics(const int32_t* lists, int64_t n, int32_t list_k, const int64_t* gt_ptr,
                         const int32_t* gt_items, const int32_t* k_list, int32_t nk, float* recall,
                         float* ndcg) {
  int32_t mk = 0;
  const std::string e = metric_args_error(n, gt_ptr, gt_items, k_list, nk, -1, &mk);
  if (!e.empty()) return fail(nullptr, FRECSYS_ERR_INVALID, "list_metrics: " + e);
  if (list_k < mk)
    return fail(nullptr, FRECSYS_ERR_INVALID, "list_metrics: list_k is below the largest cut-off");
  if (n > 0 && (!lists || !recall || !ndcg))
    return fail(nullptr, FRECSYS_ERR_INVALID, "list_metrics: bad arguments (null lists / outputs)");
  const MetricTables& tab = metric_tables();
  std::vector<int64_t> sp;
  std::vector<int32_t> sg;
  sorted_ground_truth(n, gt_ptr, gt_items, &sp, &sg);
  std::vector<uint8_t> hit((size_t)mk);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* g0 = sg.data() + sp[(size_t)i];
    const int32_t* g1 = sg.data() + sp[(size_t)i + 1];
    const int64_t g = g1 - g0;
    const int32_t* list = lists + i * list_k;
    for (int32_t j = 0; j < mk; ++j)  // -1: an empty slot, never a hit
      hit[(size_t)j] = list[j] >= 0 && std::binary_search(g0, g1, list[j]);
    for (int32_t q = 0; q < nk; ++q) {
      const int32_t kq = k_list[q];  // <= mk <= list_k
      double hits = 0.0, dcg = 0.0;
      for (int32_t j = 0; j < kq; ++j)
        if (hit[(size_t)j]) {
          hits += 1.0;
          dcg += tab.gain[j];
        }
      const double norm = tab.idcg[std::min<int64_t>(kq, g)];
      recall[i * nk + q] = (float)(hits / std::min<float>((float)kq, (float)g));
      ndcg[i * nk + q] = (float)(dcg / norm);
    }
  }
  return FRECSYS_OK;
}

int frecsys_position_metrics(const int32_t* rank, const int64_t* gt_ptr, const int32_t* eligible,
                             int64_t n_rows, float* mrr, float* auc) {
  const std::string w = "position_metrics: ";
  if (n_rows < 0 || !gt_ptr)
    return fail(nullptr, FRECSYS_ERR_INVALID, w + "bad arguments (null gt_ptr, n < 0)");
  const int64_t n = n_rows;
  const std::string e = gt_ptr_error(n, gt_ptr);
  if (!e.empty()) return fail(nullptr, FRECSYS_ERR_INVALID, w + e);
  if (n > 0 && (!rank || !eligible || !mrr || !auc))
    return fail(nullptr, FRECSYS_ERR_INVALID,
                w + "bad arguments (null ranks / eligible / outputs)");
  for (int64_t i = 0; i < n; ++i)  // (so a row never has more distinct ranks than eligible items)
    for (int64_t p = gt_ptr[i]; p < gt_ptr[i + 1]; ++p)
      if (rank[p] < -1 || rank[p] >= eligible[i])
        return fail(nullptr, FRECSYS_ERR_INVALID,
                    w + "rank " + std::to_string(rank[p]) + " of row " + std::to_string(i) +
                        " outside [-1, eligible)");
  std::vector<int32_t> R;
  for (int64_t i = 0; i < n; ++i) {
    R.assign(rank + gt_ptr[i], rank + gt_ptr[i + 1]);
    std::sort(R.begin(), R.end());
    R.erase(std::unique(R.begin(), R.end()), R.end());
    if (!R.empty() && R[0] < 0) R.erase(R.begin());
    const int64_t g = (int64_t)R.size(), M = eligible[i];  // g <= M
    int64_t inv = 0;
    for (int64_t q = 0; q < g; ++q) inv += (int64_t)R[(size_t)q] - q;
    mrr[i] = g ? (float)(1.0 / (double)((int64_t)R[0] + 1)) : 0.0f;
    auc[i] = g == 0   ? 0.0f
             : M == g ? 1.0f
                      : (float)(1.0 - (double)inv / ((double)g * (double)(M - g)));
  }
  return FRECSYS_OK;
}

int frecsys_metric_cvar(const float* values, int64_t n, const float* alphas, int32_t na,
                        float* out) {
  if (n < 0 || na < 0 || (n > 0 && !values) || (na > 0 && (!alphas || !out)))
    return fail(nullptr, FRECSYS_ERR_INVALID, "metric_cvar: bad arguments");
  // EvaluationResult::cvar (evaluation.h:83-102), verbatim
  std::vector<float> ms(values, values + n);
  std::sort(ms.begin(), ms.end());
  for (int32_t j = 0; j < na; ++j) out[j] = 0.0f;
  int64_t counter = 0;
  float acc = 0.0f;
  for (int64_t i = 0; i < n; ++i) {
    acc += ms[(size_t)i];
    for (int64_t j = counter; j < na; ++j) {
      const int pos = (int)((float)n * alphas[j]);
      if (pos == i) {
        out[counter] = acc / (float)(i + 1);
        counter++;
      }
    }
  }
  return FRECSYS_OK;
}

// Queries up to which frecsys_audience takes the thin-query kernel when
// FRECSYS_AUDIENCE_THIN_MAX is unset (the sweep it comes from).
constexpr int64_t kAudienceThinMaxDefault = 4096;

int frecsys_audience_plan(int32_t dim, int64_t n_users, int64_t n, int32_t k, int32_t cus,
                          int32_t exclude, frecsys_audience_plan_t* out) {
  const int Dp = padded_dim(dim);
  if (Dp == 0 || n_users < 1 || n < 1 || k < 1 || k > 1024 || cus < 1 ||
      (exclude != 0 && exclude != 1) || !out)
    return fail(nullptr, FRECSYS_ERR_INVALID, "frecsys_audience_plan: bad arguments");
  int64_t thin_max = kAudienceThinMaxDefault;
  if (const char* v = getenv("FRECSYS_AUDIENCE_THIN_MAX")) thin_max = std::max<long long>(0, atoll(v));
  int want_splits = 0;
  if (const char* v = getenv("FRECSYS_RECOMMEND_SPLITS")) want_splits = std::max(0, atoi(v));
  const int64_t m = n_users;
  const size_t budget = workspace_budget();
  const size_t bits = exclude ? (size_t)recommend_words(m) * 4 : 0;  // history bits per query
  frecsys_audience_plan_t p{};
  size_t per_row = 0;
  int64_t nb = 0;
  if (n <= thin_max) {
    // about 4 workgroups per CU over the passes, one chunk per split at least;
    // halved while one query's lists do not fit the budget
    const int QT = audience_queries_per_pass();
    p.thin = 1;
    p.chunk_rows = audience_chunk_rows();
    p.slots = audience_slots(k);
    const int64_t chunks = (m + p.chunk_rows - 1) / p.chunk_rows, passes = (n + QT - 1) / QT;
    int64_t splits = want_splits ? want_splits : (4 * (int64_t)cus + passes - 1) / passes;
    splits = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(splits, chunks), 65535));
    const auto bytes = [&](int64_t s) {
      return (size_t)s * p.slots * 8 + (size_t)s * 4 +
             (size_t)audience_reduce_lists((int)s, k) * ((size_t)k * 8 + 4) + (size_t)k * 8 + bits;
    };
    while (splits > 1 && bytes(splits) > budget) splits = (splits + 1) / 2;
    p.splits = (int32_t)splits;
    p.merge_rounds = audience_merge_rounds(p.splits, k);
    per_row = bytes(splits);
    nb = std::max<int64_t>(1, (int64_t)(budget / per_row));
    p.queries_per_pass = (int32_t)std::min<int64_t>(QT, nb);
    if (nb < n && nb >= QT) nb -= nb % QT;  // whole passes but in the last batch
  } else {
    // scan_plan's arithmetic (serve.hip) with the caller's CU count
    const int max_splits = recommend_max_splits(k, m);
    const int64_t row_blocks = (n + 63) / 64;
    int64_t splits = std::min<int64_t>(max_splits, (2 * (int64_t)cus + row_blocks - 1) / row_blocks);
    if (want_splits) splits = std::min(max_splits, want_splits);
    p.splits = (int32_t)std::max<int64_t>(1, splits);
    p.chunk_rows = 128;
    p.slots = recommend_cap(k);
    p.merge_rounds = 1;
    per_row = (size_t)p.splits * p.slots * 8 + (size_t)p.splits * 4 + (size_t)k * 8 + bits;
    nb = std::max<int64_t>(1, (int64_t)(budget / per_row));
    p.queries_per_pass = (int32_t)std::min<int64_t>(64, nb);
    if (nb < n && nb >= 64) nb &= ~(int64_t)63;  // whole 64-row blocks but in the last batch
  }
  p.passes = (int32_t)((n + p.queries_per_pass - 1) / p.queries_per_pass);
  p.rows_per_batch = std::min(nb, n);
  p.workspace_bytes = (int64_t)((size_t)p.rows_per_batch * per_row);
  *out = p;
  return FRECSYS_OK;
}

int frecsys_bf16_round(const float* in, int64_t n, float* out) {
  if (n < 0 || (n > 0 && (!in || !out)))
    return fail(nullptr, FRECSYS_ERR_INVALID, "frecsys_bf16_round: bad arguments");
  for (int64_t i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, in + i, 4);
    u = bf16_round_bits(u) << 16;
    std::memcpy(out + i, &u, 4);
  }
  return FRECSYS_OK;
}

double frecsys_two_stage_bound(int32_t dim, double query_norm, double item_norm_max) {
#pragma clang fp contract(off)
  const int Dp = padded_dim(dim);
  if (Dp == 0) return std::nan("");
  return two_stage_c(Dp) * query_norm * item_norm_max;
}

}  // extern "C"
