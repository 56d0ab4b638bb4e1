/*
 * frecsys_model.h -- C-ABI of libfrecsys_model.so: the reference's model
 * surface (the abstract frecsys::Recommender, recommender.h:40-59, and the
 * model constructors ials.h:39-42, ialspp.h, safer2.h:37-43, safer2pp.h,
 * erm_mf.h:37-40, cvar_mf.h:36-38) for callers that cannot link C++
 * (ctypes / cgo / JNI), driving the same C++ classes as run_model.
 *
 *   frecsys_model_create      -- run_model's Dataset(train) + get_model()
 *                                (run_model.cc:43-123, 233-241): the model is
 *                                sized max_user + 1 / max_item + 1 of the
 *                                tuples, seeded init of U then V
 *   frecsys_model_initialize  -- the Initialize(train) calls of
 *                                run_model.cc:246-257 (SAFER2, SAFER2++,
 *                                ERM-MF, CVaR-MF; no-op for iALS / iALS++)
 *   frecsys_model_train       -- `recommender->Train(train)` of the epoch
 *                                loop (run_model.cc:258-266), `epochs` times
 *   frecsys_model_context     -- the device context (include/frecsys_hip.h)
 *                                the model runs on: embeddings, timers
 *   frecsys_model_save / _load -- checkpoints: exact resume, serve-only load,
 *                                warm start (no reference counterpart)
 *
 * Conditions the reference treats as fatal (a failed LLT, ials.h:141; NaN
 * losses, ials.h:291-296) end the process as they do there.  The tuples
 * passed to frecsys_model_create are copied; nothing is retained.
 */
#ifndef FRECSYS_MODEL_H_
#define FRECSYS_MODEL_H_

#include <stdint.h>

#include "frecsys_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct frecsys_model frecsys_model;

/* The run_model flags (run_model.cc:129-230), one field each. */
typedef struct {
  const char* model_name; /* ials | ialspp | safer2 | safer2pp | erm_mf | cvar_mf */
  int32_t dim;
  float l2_reg;
  float l2_reg_exp;
  float uobs_weight;
  float stdev;
  float alpha;
  float bandwidth;
  float stepsize;
  float sampling_ratio;
  int32_t block_size;
  int32_t xi_iterations;
  int32_t pd_iterations;
  int32_t use_epanechnikov;
  int32_t use_snr;
  int32_t print_train_stats;
  int32_t print_residual_stats;
  int32_t print_var_stats;
  int64_t seed;           /* -1: std::random_device, as the reference */
  int32_t device;         /* HIP ordinal; -1: LOCAL_RANK or the current device */
  int32_t parity_quirks;  /* SURVEY App. A.1 */
  int32_t world;          /* 0: WORLD_SIZE (1 if unset) */
  int32_t rank;           /* -1: RANK */
  const uint8_t* comm_id; /* world > 1: the 128-byte RCCL id of rank 0
                             (frecsys_comm_unique_id); NULL: FRECSYS_COMM_FILE */
  /* --use_cg / --cg_error_tolerance / --cg_max_iterations (run_model.cc:172):
   * ials and safer2 solve by conjugate gradients (frecsys_solve_side_cg);
   * erm_mf with use_cg is FRECSYS_ERR_UNSUPPORTED (its BiCGSTAB path is not
   * built); ialspp, safer2pp and cvar_mf take no such arguments in the
   * reference and ignore them. */
  int32_t use_cg;
  float cg_error_tolerance;
  int32_t cg_max_iterations;
} frecsys_model_config;

/* The run_model defaults (model_name NULL: must be set by the caller). */
void frecsys_model_config_default(frecsys_model_config* cfg);
/* users[k], items[k]: the k-th training tuple (file order). */
int frecsys_model_create(const frecsys_model_config* cfg, const int32_t* users,
                         const int32_t* items, int64_t n_tuples, frecsys_model** out);
int frecsys_model_initialize(frecsys_model* m);
int frecsys_model_train(frecsys_model* m, int32_t epochs);
frecsys_ctx* frecsys_model_context(frecsys_model* m);
/* GetMeanWeight() of SAFER2 / SAFER2++ (safer2.h:815-817); alpha for ERM-MF. */
float frecsys_model_mean_weight(const frecsys_model* m);
/* The dual state of ERM-MF / CVaR-MF / SAFER2 (-MF++): weights[n_users] =
 * the omega the last Train() (or Initialize()) left -- the weights its
 * half-steps used (safer2.h:272-290) --, losses[n_users] = user_loss_ of the
 * last ComputeUserLoss, item_reg[n_items] = item_reg_ (safer2.h:831-837),
 * xi = the current xi (SAFER2 / SAFER2++; NaN otherwise).  Any pointer may be
 * NULL; iALS has none of these (FRECSYS_ERR_INVALID for weights/item_reg). */
int frecsys_model_dual_state(const frecsys_model* m, float* weights, float* losses,
                             float* item_reg, float* xi);
/* The k best items for n trained users (users[i]: a row of U; any order,
 * repeats allowed) with their scores, items / scores: host [n * k] (scores
 * may be NULL); exclude_seen != 0 drops each user's training history (the
 * model must have been trained: Train() loads it), item_mask: host
 * [n_items] bytes, non-zero = candidate, or NULL.  Ranking, ties, the -1 /
 * -FLT_MAX fill and the errors are frecsys_recommend's (frecsys_hip.h); no
 * reference counterpart beyond EvaluateUser's scoring, recommender.h:132-199. */
int frecsys_model_recommend(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                            int32_t exclude_seen, const uint8_t* item_mask,
                            int32_t* items, float* scores);
/* The same for n unseen users given by their histories (hist_items[hist_ptr[i]
 * .. hist_ptr[i+1]): item ids of user i, hist_ptr[0] = 0): the model's own
 * fold-in projection (the first half of its EvaluateDataset: ials.h:148-174
 * and the variants; 8 epochs of block steps for iALS++ / SAFER2++,
 * ialspp.h:148-206) into the EVAL side of its context, then the ranking of
 * those rows; exclude_seen drops the given history. */
int frecsys_model_recommend_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                    const int32_t* hist_items, int64_t n, int32_t k,
                                    int32_t exclude_seen, const uint8_t* item_mask,
                                    int32_t* items, float* scores);
/* The two calls above by retrieve-then-rank (frecsys_recommend_two_stage,
 * frecsys_hip.h, where the bf16 scan, the pool, the exact re-scoring and the
 * certificate are defined): 1 <= k <= pool <= 1024, pool = 0: the default;
 * exact != 0 re-runs the rows that stage 2 cannot certify through
 * frecsys_recommend's scan, so that items / scores are
 * frecsys_model_recommend's bit for bit on every row; certified: host [n] or
 * NULL, 0 / 1 / 2 per row.  The errors are frecsys_model_recommend's and
 * frecsys_recommend_two_stage's. */
int frecsys_model_recommend_two_stage(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                                      int32_t pool, int32_t exact, int32_t exclude_seen,
                                      const uint8_t* item_mask, int32_t* items, float* scores,
                                      uint8_t* certified);
int frecsys_model_recommend_two_stage_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                              const int32_t* hist_items, int64_t n, int32_t k,
                                              int32_t pool, int32_t exact, int32_t exclude_seen,
                                              const uint8_t* item_mask, int32_t* items,
                                              float* scores, uint8_t* certified);
/* Diversified lists for n trained users: greedy maximal-marginal-relevance
 * (MMR) re-ranking of each user's `pool` best items down to k
 * (frecsys_recommend_diverse, frecsys_hip.h, where the pool, the relevance,
 * the cosine chain, the greedy steps, the tie order and the outputs are fixed
 * to the bit): frecsys_model_recommend(k = pool) followed by
 * frecsys_mmr_select on its lists against the model's item table, with the
 * pools never leaving the device.  1 <= k <= pool <= 1024; lam in [0, 1]
 * (1: frecsys_model_recommend(k)'s lists); raw_scores != 0: relevance = the
 * score itself instead of its min-max normalisation over the pool;
 * exclude_seen and item_mask as in frecsys_model_recommend.  items / scores:
 * host [n * k]; mmr: host [n * k] or NULL, the MMR value of each selection.
 * The errors are frecsys_recommend_diverse's, reported before any device
 * call. */
int frecsys_model_recommend_diverse(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                                    int32_t pool, float lam, int32_t raw_scores,
                                    int32_t exclude_seen, const uint8_t* item_mask,
                                    int32_t* items, float* scores, float* mmr);
/* The same for n unseen users given by their histories (as
 * frecsys_model_recommend_fold_in): the model's fold-in projection into the
 * EVAL side of its context, where the projected rows stay, then the
 * diversified lists of those rows; exclude_seen drops the given history.  A
 * bad argument is reported before anything is projected. */
int frecsys_model_recommend_diverse_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                            const int32_t* hist_items, int64_t n, int32_t k,
                                            int32_t pool, float lam, int32_t raw_scores,
                                            int32_t exclude_seen, const uint8_t* item_mask,
                                            int32_t* items, float* scores, float* mmr);
/* The same selection from caller-supplied pools (frecsys_diversify,
 * frecsys_hip.h; its errors): lists / list_scores: host [n * pool] item ids
 * (negative: an empty slot; repeats are candidates of their own) and scores
 * from anywhere -- frecsys_model_rank_candidates, frecsys_model_similar_items,
 * another retriever --, diversified against the model's item table. */
int frecsys_model_diversify(frecsys_model* m, const int32_t* lists, const float* list_scores,
                            int64_t n, int32_t pool, int32_t k, float lam, int32_t raw_scores,
                            int32_t* items, float* scores, float* mmr);
/* The DPP counterparts of the three calls above (frecsys_recommend_dpp,
 * frecsys_diversify_dpp, frecsys_hip.h, where the quality w = dpp_exp2(theta
 * rel), the greedy steps of the incremental Cholesky, the fallback below eps,
 * the tie order and the outputs are fixed to the bit):
 * frecsys_model_recommend(k = pool) followed by frecsys_dpp_select on its
 * lists against the model's item table, with the pools never leaving the
 * device.  1 <= k <= pool <= 1024; theta finite and >= 0 (0: pure diversity);
 * eps in (0, 1]; raw_scores, exclude_seen and item_mask as for the MMR calls.
 * items / scores: host [n * k]; gain: host [n * k] or NULL, the gain of each
 * selection (0 in the fallback).  The errors are frecsys_recommend_dpp's /
 * frecsys_diversify_dpp's, reported before any device call and, for the
 * fold-in form, before anything is projected. */
int frecsys_model_recommend_dpp(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                                int32_t pool, float theta, float eps, int32_t raw_scores,
                                int32_t exclude_seen, const uint8_t* item_mask, int32_t* items,
                                float* scores, float* gain);
int frecsys_model_recommend_dpp_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                        const int32_t* hist_items, int64_t n, int32_t k,
                                        int32_t pool, float theta, float eps, int32_t raw_scores,
                                        int32_t exclude_seen, const uint8_t* item_mask,
                                        int32_t* items, float* scores, float* gain);
int frecsys_model_diversify_dpp(frecsys_model* m, const int32_t* lists, const float* list_scores,
                                int64_t n, int32_t pool, int32_t k, float theta, float eps,
                                int32_t raw_scores, int32_t* items, float* scores, float* gain);
/* List quality of a serving configuration for trained users
 * (frecsys_rank_quality, frecsys_hip.h: the definitions of ILD, novelty and
 * exposure, the tolerance and what is exact are stated there): the lists are
 * frecsys_model_recommend(k = max k_list)'s when pool == 0 (lam ignored,
 * raw_scores 0) and frecsys_model_recommend_diverse(k = max k_list, pool, lam,
 * raw_scores)'s when pool > 0, measured on the device.  ild, novelty: host
 * [n * nk]; exposure: host int64 [nk * n_items]; item_weight: host [n_items]
 * with novelty, NULL without.  A ground truth (gt_ptr / gt_items, row i belongs
 * to users[i]) is optional: with it recall and ndcg [n * nk] are both given and
 * hold frecsys_model_evaluate's values of the same lists; without it gt_ptr,
 * gt_items, recall and ndcg are NULL.  summary (or NULL): double
 * [(6 + 2 na) nk] -- mean ILD [nk] and mean novelty [nk] (double sums of the
 * per-row values in row order, over n), coverage [nk] and Gini [nk] of each
 * exposure row among the items of item_mask (frecsys_exposure_summary), then
 * frecsys_model_evaluate's summary widened: mean recall, mean ndcg, recall
 * CVaR [na][nk], ndcg CVaR [na][nk]; a block whose output was not asked for
 * holds 0.  FRECSYS_ERR_INVALID, every check before any device work:
 * frecsys_rank_quality's cases in this layer's words, raw_scores outside
 * {0, 1} or without a pool, a bad alpha_list, frecsys_model_evaluate's
 * ground-truth cases, exclude_seen on a serve-only model. */
int frecsys_model_evaluate_quality(frecsys_model* m, const int64_t* users, int64_t n,
                                   const int32_t* k_list, int32_t nk, int32_t pool, float lam,
                                   int32_t raw_scores, const float* item_weight,
                                   const int64_t* gt_ptr, const int32_t* gt_items,
                                   const float* alpha_list, int32_t na, int32_t exclude_seen,
                                   const uint8_t* item_mask, float* ild, float* novelty,
                                   float* recall, float* ndcg, int64_t* exposure,
                                   double* summary);
/* The same for n unseen users given by their histories (CSR), as
 * frecsys_model_recommend_fold_in: the model's fold-in projection, then the
 * quality of the projected rows' lists; exclude_seen drops the given history.
 * A bad argument is reported before anything is projected. */
int frecsys_model_evaluate_quality_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                           const int32_t* hist_items, int64_t n,
                                           const int32_t* k_list, int32_t nk, int32_t pool,
                                           float lam, int32_t raw_scores,
                                           const float* item_weight, const int64_t* gt_ptr,
                                           const int32_t* gt_items, const float* alpha_list,
                                           int32_t na, int32_t exclude_seen,
                                           const uint8_t* item_mask, float* ild, float* novelty,
                                           float* recall, float* ndcg, int64_t* exposure,
                                           double* summary);
/* The same measures of caller-supplied lists [n * list_k] (negative: an empty
 * slot) against the model's item table (frecsys_lists_quality; its errors).
 * item_mask only selects the items of the summary; summary (or NULL): double
 * [4 nk], the first four blocks above. */
int frecsys_model_list_quality(frecsys_model* m, const int32_t* lists, int64_t n, int32_t list_k,
                               const int32_t* k_list, int32_t nk, const float* item_weight,
                               const uint8_t* item_mask, float* ild, float* novelty,
                               int64_t* exposure, double* summary);
/* scores[i] = the model's score of items[i] for trained user users[i] (a row
 * of U), n pairs, any order, repeats allowed; host arrays [n].  Bit for bit
 * the score frecsys_model_recommend lists for that user and item
 * (frecsys_score_pairs, frecsys_hip.h; its errors). */
int frecsys_model_score(frecsys_model* m, const int64_t* users, const int32_t* items, int64_t n,
                        float* scores);
/* Why an item scores what it does (frecsys_explain, frecsys_hip.h; its errors):
 * for trained user users[i] (n of them, repeats allowed) and each of its
 * targets tgt_items[tgt_ptr[i] .. tgt_ptr[i+1]) (tgt_ptr[0] = 0), the score
 * split exactly over the user's training history: score: host [pairs],
 * top_items / top_contrib: host [pairs * top] (top in 1..32: the largest
 * contributions with their history item ids, -1 / 0 fill), full: NULL or the
 * h contributions of every pair in CSR order.  The model supplies the solve
 * parameters of its own fold-in (omega = 1 where the fold-in uses it) against
 * the current item table and its Gramian.  `score` is therefore the score of
 * the model's EXACT projection of that history against the current item table
 * -- what frecsys_model_recommend_fold_in lists for the same history -- and not
 * frecsys_model_score's U[user] . V[item]: a trained row of U was solved
 * against the item table of the previous half-step.  iALS++ and SAFER2++ use
 * the parameters of the objective their block steps descend, so theirs is the
 * explanation of that objective's exact minimiser; their own fold-in stops
 * after 8 block epochs and is only near it.  The training CSR must be loaded
 * (the model trained here, or loaded with its tuples): FRECSYS_ERR_INVALID on
 * a serve-only model. */
int frecsys_model_explain(frecsys_model* m, const int64_t* users, int64_t n,
                          const int64_t* tgt_ptr, const int32_t* tgt_items, int32_t top,
                          float* score, int32_t* top_items, float* top_contrib, float* full);
/* The same for n unseen users given by their histories (as
 * frecsys_model_recommend_fold_in): the histories are loaded as the EVAL side
 * of the context (the projected EVAL rows of an earlier fold-in are zeroed, as
 * by any load) and target list i belongs to history row i.  Bit for bit
 * frecsys_model_explain's result for a user with the same history. */
int frecsys_model_explain_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                  const int32_t* hist_items, int64_t n, const int64_t* tgt_ptr,
                                  const int32_t* tgt_items, int32_t top, float* score,
                                  int32_t* top_items, float* top_contrib, float* full);
/* The k best of each trained user's own candidate list (users[i]: a row of U;
 * cand_items[cand_ptr[i] .. cand_ptr[i+1]): the candidates of users[i],
 * cand_ptr[0] = 0; repeats count once) with their scores, items / scores:
 * host [n * k] (scores may be NULL).  exclude_seen and item_mask as in
 * frecsys_model_recommend; ranking, ties, the -1 / -FLT_MAX fill and the
 * errors are frecsys_rank_candidates' (frecsys_hip.h). */
int frecsys_model_rank_candidates(frecsys_model* m, const int64_t* users, int64_t n,
                                  const int64_t* cand_ptr, const int32_t* cand_items, int32_t k,
                                  int32_t exclude_seen, const uint8_t* item_mask,
                                  int32_t* items, float* scores);
/* The k best users for trained items (items[i]: a row of V; n ids, any order,
 * repeats allowed, or NULL = rows 0 .. n-1): frecsys_audience (frecsys_hip.h).
 * exclude_seen != 0 drops the users who have the item in the training tuples
 * (loaded into the context here if no Train() has done it yet; a model loaded
 * without its tuples answers FRECSYS_ERR_INVALID); user_mask: host [n_users]
 * eligibility bytes or NULL; users / scores: host [n * k] (scores may be
 * NULL).  Scores -- bit for bit frecsys_model_score's --, order, ties, the -1 /
 * -FLT_MAX fill and the errors are frecsys_audience's; the arguments are
 * checked before any device call. */
int frecsys_model_audience(frecsys_model* m, const int64_t* items, int64_t n, int32_t k,
                           int32_t exclude_seen, const uint8_t* user_mask, int32_t* users,
                           float* scores);
/* The k nearest neighbours of trained items among the items (items[i]: a row
 * of V) and of trained users among the users (users[i]: a row of U), by cosine
 * (FRECSYS_SIM_COSINE in flags) or dot product; without FRECSYS_SIM_KEEP_SELF
 * a query never lists itself.  items / users: n row ids, any order, repeats
 * allowed, or NULL = rows 0 .. n-1; item_mask / user_mask: host [n_items] /
 * [n_users] eligibility bytes or NULL; ids / scores: host [n * k] (scores may
 * be NULL).  Scores, order, ties, the -1 / -FLT_MAX fill and the errors are
 * frecsys_similar's (frecsys_hip.h); the arguments are checked before any
 * device call. */
int frecsys_model_similar_items(frecsys_model* m, const int64_t* items, int64_t n, int32_t k,
                                int32_t flags, const uint8_t* item_mask, int32_t* ids,
                                float* scores);
int frecsys_model_similar_users(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                                int32_t flags, const uint8_t* user_mask, int32_t* ids,
                                float* scores);
/* The same for n unseen users given by their histories (as
 * frecsys_model_recommend_fold_in): the model's fold-in projection into the
 * EVAL side of its context, where the projected rows stay, then the ranking
 * of candidate list i for history row i; exclude_seen drops the given
 * history. */
int frecsys_model_rank_candidates_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                          const int32_t* hist_items, int64_t n,
                                          const int64_t* cand_ptr, const int32_t* cand_items,
                                          int32_t k, int32_t exclude_seen,
                                          const uint8_t* item_mask, int32_t* items,
                                          float* scores);
/* Ranking quality of n trained users (users[i]: a row of U) against their
 * ground truth (gt_items[gt_ptr[i] .. gt_ptr[i+1]): the held-out items of
 * users[i]; not empty): Recall@K and NDCG@K of frecsys_model_recommend's
 * ranking at each of the nk cut-offs of k_list, computed on the device
 * (frecsys_rank_metrics, frecsys_hip.h: the reference's RankMetrics,
 * recommender.h:152-182), recall / ndcg: host [n * nk].  summary: host
 * [(2 + 2 na) * nk] or NULL -- mean recall [nk], mean ndcg [nk], recall CVaR
 * [na][nk], ndcg CVaR [na][nk]: what EvaluationResult::show() logs, from its
 * own colwise().mean() (double sum in row order) and cvar()
 * (evaluation.h:83-102, quirks included: see frecsys_metric_cvar).
 * exclude_seen != 0 drops each user's training history from the ranking.
 * Errors are frecsys_rank_metrics', reported before any device call. */
int frecsys_model_evaluate(frecsys_model* m, const int64_t* users, int64_t n,
                           const int64_t* gt_ptr, const int32_t* gt_items,
                           const int32_t* k_list, int32_t nk, const float* alpha_list,
                           int32_t na, int32_t exclude_seen, float* recall, float* ndcg,
                           float* summary);
/* The same for n unseen users given by their histories (as
 * frecsys_model_recommend_fold_in): the model's fold-in projection into the
 * EVAL side of its context, where the projected rows stay, then the metrics
 * of those rows; ground-truth row i belongs to history row i; exclude_seen
 * drops the given history.  This is the reference's EvaluateDataset
 * (recommender.h:78-199) with the ranking and the metrics on the device. */
int frecsys_model_evaluate_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                   const int32_t* hist_items, int64_t n,
                                   const int64_t* gt_ptr, const int32_t* gt_items,
                                   const int32_t* k_list, int32_t nk,
                                   const float* alpha_list, int32_t na,
                                   int32_t exclude_seen, float* recall, float* ndcg,
                                   float* summary);
/* Full-catalogue positions of the ground truth of n trained users
 * (frecsys_rank_positions, frecsys_hip.h): where frecsys_model_recommend would
 * list each held-out item if its k were large enough, and per user the
 * reciprocal rank of the best one and the AUC.  rank: host [gt_ptr[n]];
 * eligible, mrr, auc: host [n]; each may be NULL, not all four.  item_mask:
 * host [n_items] or NULL.  summary: host [2 + 2 na] or NULL (it needs mrr and
 * auc) -- mean mrr, mean auc, mrr CVaR [na], auc CVaR [na], by
 * frecsys_model_evaluate's own mean (double sum in row order) and cvar(),
 * quirks included.  Errors are frecsys_rank_positions', reported before any
 * device call.  The _fold_in form projects the n histories into the EVAL side
 * first, as frecsys_model_evaluate_fold_in does. */
int frecsys_model_evaluate_ranks(frecsys_model* m, const int64_t* users, int64_t n,
                                 const int64_t* gt_ptr, const int32_t* gt_items,
                                 const float* alpha_list, int32_t na, int32_t exclude_seen,
                                 const uint8_t* item_mask, int32_t* rank, int32_t* eligible,
                                 float* mrr, float* auc, float* summary);
int frecsys_model_evaluate_ranks_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                         const int32_t* hist_items, int64_t n,
                                         const int64_t* gt_ptr, const int32_t* gt_items,
                                         const float* alpha_list, int32_t na,
                                         int32_t exclude_seen, const uint8_t* item_mask,
                                         int32_t* rank, int32_t* eligible, float* mrr,
                                         float* auc, float* summary);
/* frecsys_model_evaluate restricted to caller-supplied candidate lists
 * (second-stage evaluation): Recall@K / NDCG@K of the lists
 * frecsys_model_rank_candidates returns with k = max(k_list), computed on the
 * device without the lists leaving it (frecsys_rank_candidates_metrics,
 * frecsys_hip.h).  Candidate list i (cand_items[cand_ptr[i] .. cand_ptr[i+1]))
 * and ground-truth row i belong to users[i]; a ground-truth item outside the
 * list, masked or in the excluded history is never a hit.  item_mask: host
 * [n_items] or NULL.  recall, ndcg and summary have exactly
 * frecsys_model_evaluate's layout and arithmetic.  Errors are
 * frecsys_rank_candidates_metrics', reported before any device call.  The
 * _fold_in form projects the n histories into the EVAL side first, as
 * frecsys_model_evaluate_fold_in does. */
int frecsys_model_evaluate_candidates(frecsys_model* m, const int64_t* users, int64_t n,
                                      const int64_t* cand_ptr, const int32_t* cand_items,
                                      const int64_t* gt_ptr, const int32_t* gt_items,
                                      const int32_t* k_list, int32_t nk, const float* alpha_list,
                                      int32_t na, int32_t exclude_seen, const uint8_t* item_mask,
                                      float* recall, float* ndcg, float* summary);
int frecsys_model_evaluate_candidates_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                              const int32_t* hist_items, int64_t n,
                                              const int64_t* cand_ptr, const int32_t* cand_items,
                                              const int64_t* gt_ptr, const int32_t* gt_items,
                                              const int32_t* k_list, int32_t nk,
                                              const float* alpha_list, int32_t na,
                                              int32_t exclude_seen, const uint8_t* item_mask,
                                              float* recall, float* ndcg, float* summary);
/* Sampled evaluation: each user's distinct ground truth ranked against n_neg
 * negatives drawn on the device by the generator of frecsys_sample_negatives
 * with this seed (side row id = users[i]; history row i has id i in the
 * _fold_in form), or against the user's whole pool where that is small
 * (frecsys_sampled_metrics, frecsys_hip.h).  The price of an evaluation drops
 * from users x items scores to users x (n_neg + ground truth); the values are
 * NOT estimates of frecsys_model_evaluate's full-catalogue metrics and the two
 * are not interchangeable (Krichene & Rendle, KDD 2020).  Outputs, summary
 * and exclude_seen as in frecsys_model_evaluate; errors are
 * frecsys_sampled_metrics', reported before any device call. */
int frecsys_model_evaluate_sampled(frecsys_model* m, const int64_t* users, int64_t n,
                                   const int64_t* gt_ptr, const int32_t* gt_items, int32_t n_neg,
                                   uint64_t seed, const int32_t* k_list, int32_t nk,
                                   const float* alpha_list, int32_t na, int32_t exclude_seen,
                                   const uint8_t* item_mask, float* recall, float* ndcg,
                                   float* summary);
int frecsys_model_evaluate_sampled_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                           const int32_t* hist_items, int64_t n,
                                           const int64_t* gt_ptr, const int32_t* gt_items,
                                           int32_t n_neg, uint64_t seed, const int32_t* k_list,
                                           int32_t nk, const float* alpha_list, int32_t na,
                                           int32_t exclude_seen, const uint8_t* item_mask,
                                           float* recall, float* ndcg, float* summary);
/* ---- checkpoints (format, version 1: safer2-recommender_amd/include/frecsys/
 * checkpoint.h and DESIGN.md 3.16) ----
 *
 * frecsys_model_save writes the whole model to `path`: configuration, U, V,
 * the dual state of frecsys_model_dual_state, the state that lives across
 * Train() calls (xi, the SNR generator, the epoch count) and, unless
 * FRECSYS_SAVE_NO_DATA is set, the training tuples.  The file is written
 * beside `path` under a temporary name, flushed, fsynced and renamed over
 * `path`; a failure removes the temporary file and leaves an existing `path`
 * as it was.  At most one table is held on the host at a time.  Any rank of
 * a multi-rank model may save: every rank holds the full tables and vectors
 * and the file holds nothing rank-specific.  FRECSYS_ERR_IO: open / write /
 * rename failed. */
#define FRECSYS_SAVE_NO_DATA 1 /* leave USERS / ITEMS out */
int frecsys_model_save(frecsys_model* m, const char* path, int32_t flags);
/* A model from a file.  The whole file is validated first, on the host
 * (FRECSYS_ERR_INVALID for a malformed file, FRECSYS_ERR_IO for an open or
 * read failure; FRECSYS_ERR_NO_DEVICE only for a good file).
 *   cfg NULL: the stored configuration, default device / world / rank /
 *     comm_id; else cfg as given (frecsys_model_file_info, edit, load):
 *     model_name and dim must be the file's, parity_quirks too unless
 *     FRECSYS_LOAD_TABLES_ONLY.
 *   flags 0, resume: the tuples come from the file (users NULL) or from the
 *     caller, whose count and checksum must be the stored ones.  The model is
 *     in exactly the saved state and initialised (frecsys_model_initialize is
 *     a no-op), its training CSR loaded, so exclude_seen works before any
 *     Train(); frecsys_model_epochs continues; the next Train() is the saved
 *     run's next one, bit for bit.
 *   flags 0, users NULL, a file without tuples: serve-only.  Tables, Gramians
 *     and dual state are restored; frecsys_model_train and every call on
 *     trained users with exclude_seen != 0 return FRECSYS_ERR_INVALID;
 *     everything else works (the fold-in calls exclude the history they are
 *     given; frecsys_model_initialize is the same no-op).
 *   FRECSYS_LOAD_TABLES_ONLY, warm start: the caller's tuples are required
 *     and may span more users / items than the file (not fewer).  The model
 *     is what frecsys_model_create makes of them, seeded init included, with
 *     rows [0, stored n) of U and V replaced from the file; no dual state,
 *     epochs 0, frecsys_model_initialize as for a new model. */
#define FRECSYS_LOAD_TABLES_ONLY 1 /* warm start: U and V only */
int frecsys_model_load(const char* path, const frecsys_model_config* cfg, const int32_t* users,
                       const int32_t* items, int64_t n_tuples, int32_t flags,
                       frecsys_model** out);
typedef struct {
  char model_name[16];
  frecsys_model_config config; /* config.model_name points at model_name above */
  int64_t n_users, n_items, n_tuples, epochs_trained;
  uint64_t flags; /* bit 0: the file holds the training tuples */
  uint64_t tuples_checksum;
  uint32_t version;
} frecsys_model_file_info_t; /* _t: a C typedef cannot share the function's name */
/* What a file holds.  Host only: no device, no context.  verify = 0: header,
 * directory (bounds, alignment, overlap, section sizes) and CONFIG; verify
 * != 0: every section's checksum, the zero gaps and the tuple ids too. */
int frecsys_model_file_info(const char* path, int32_t verify, frecsys_model_file_info_t* info);
/* Train() calls so far, those before a resumed model's save included. */
int64_t frecsys_model_epochs(const frecsys_model* m);
void frecsys_model_destroy(frecsys_model* m);
const char* frecsys_model_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FRECSYS_MODEL_H_ */
