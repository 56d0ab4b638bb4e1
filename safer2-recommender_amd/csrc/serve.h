// serve.h -- what the two host units of the ranking and evaluation calls
// share, one copy each: serve.hip (the calls that take a context and drive the
// device) and serve_host.hip (the context-free host arithmetic, which defines
// what is not inline here).  Internal header.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "ctx.h"

namespace frecsys_hip {

// Hidden, as ctx.h's internals: the library's dynamic symbols stay the C-ABI.
#pragma GCC visibility push(hidden)

// The arguments every MMR call checks first: 1 <= k <= pool <= 1024, lam in
// [0, 1] (a NaN fails both comparisons), the flags.  c may be nullptr.
int check_diversify(frecsys_ctx* c, const std::string& w, int32_t k, int32_t pool, float lam,
                    int32_t flags, int32_t known_flags);

// The arguments every DPP call checks first: the MMR calls' k, pool and flags,
// then theta finite and >= 0 and eps in (0, 1] (a NaN fails both comparisons).
int check_dpp(frecsys_ctx* c, const std::string& w, int32_t k, int32_t pool, float theta, float eps,
              int32_t flags, int32_t known_flags);

// A pool array [n][pool] against a catalogue of m items: ids below m, finite
// scores in the filled slots and, in normalised mode, a finite max - min per
// row; "" when fine.
std::string pool_error(const int32_t* lists, const float* list_scores, int64_t n, int32_t pool,
                       int64_t m, bool raw);

// What the quality calls add to a ranking: the cut-offs, the item weights of
// novelty (or nullptr) and where the results go (host; each may be nullptr).
struct QualityRequest {
  const int32_t* k_list;
  int32_t nk;
  const float* item_weight;
  float* ild;
  float* novelty;
  int64_t* exposure;
};

// The arguments every quality call checks, in this order: the cut-offs (each in
// [1, max_k]), the outputs (`others`: the call has outputs beside these three),
// novelty and its weights (one with the other, every weight finite); "" when
// fine.  tools/model_capi.cc restates these checks in the model layer's words,
// in the same order: the two lists stay in step.
std::string quality_args_error(const QualityRequest& q, int32_t max_k, int64_t n_items,
                               bool others);
inline int32_t max_cutoff(const int32_t* k_list, int32_t nk) {
  return *std::max_element(k_list, k_list + nk);
}

// Caller lists [n][list_k] of a quality call: n >= 0, the pointer, n * list_k
// within int64, every id below m (negative: an empty slot); "" when fine.
std::string lists_error(const int32_t* lists, int64_t n, int32_t list_k, int64_t m);

// gain[j] = 1 / log2(j + 2) and its sequential prefix idcg[m] = gain[0] + ...
// + gain[m-1] (idcg[0] = 0), in double with the host's std::log2: the terms
// and the norm of RankMetrics (recommender.h:152-182) in its own order.
struct MetricTables {
  double gain[kMetricMaxK];
  double idcg[kMetricMaxK + 1];
};
const MetricTables& metric_tables();

// The argument checks the metric calls share (gt_ptr starts at 0, is monotone
// and has no empty row); "" when fine.  n_items < 0: no upper bound on the ids.
std::string metric_args_error(int64_t n, const int64_t* gt_ptr, const int32_t* gt_items,
                              const int32_t* k_list, int32_t nk, int64_t n_items,
                              int32_t* max_k);

// The ground truth as sets: every row ascending and distinct.  Rows are sorted
// in place in a copy (a row already strictly ascending is left alone), on host
// threads over nnz-balanced row ranges when there is enough of it, then closed
// up over the dropped repeats; the thread count never changes the result.
void sorted_ground_truth(int64_t n, const int64_t* gt_ptr, const int32_t* gt_items,
                         std::vector<int64_t>* sp, std::vector<int32_t>* sg);

// Bytes the regions of a row batch may take: 256 MiB, or the knob (read per call).
inline size_t workspace_budget() {
  int64_t ws_mb = 256;
  if (const char* v = getenv("FRECSYS_RECOMMEND_WS_MB")) ws_mb = std::max(1, atoi(v));
  return (size_t)ws_mb << 20;
}

// Whole-pool rule of a sampled row with pool size E among M maskable ids.
inline bool whole_pool_row(int64_t n_neg, int64_t E, int64_t M) {
  return 2 * n_neg > E || 64 * E < M;
}

#pragma GCC visibility pop

}  // namespace frecsys_hip
