// model_base.h -- state and helpers shared by the four GPU model classes.
//
// Host-resident: the small per-user vectors of the reference models
// (user_loss_, dual_weight_, user_history_size_, item_reg_; safer2.h:841-847)
// and the print flags.  Device-resident (DeviceContext): U, V, Gramians,
// the CSR of the training set.  The static per-entity entry points
// (Project / ProjectU / ProjectV of the reference) run on the GPU through a
// one-row context (ProjectOnDevice).
#pragma once

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "frecsys/dataset.h"
#include "frecsys/device.h"
#include "frecsys/evaluation.h"
#include "frecsys/logging.h"
#include "frecsys/recommender.h"
#include "frecsys/types.h"

namespace frecsys {
namespace detail {

class DeviceModel : public Recommender {
 public:
  DeviceModel(int dim, int num_users, int num_items, float stdev, const DeviceOptions& opts)
      : dim_(dim), num_users_(num_users), num_items_(num_items), opts_(opts) {
    dev_ = std::make_unique<DeviceContext>(dim, num_users, num_items, opts);
    // adjusted_stdev = stdev / sqrt(dim); U then V from one mt19937
    // (ials.h:47-51 / recommender.h:61-67)
    dev_->InitEmbeddings(opts.seed, stdev);
  }

  void SetPrintTrainStats(const bool v) override { print_trainstats_ = v; }
  void SetPrintResidualStats(const bool v) override { print_residualstats_ = v; }
  void SetPrintVarStats(const bool v) override { print_varstats_ = v; }

  // Host copies of the device embeddings (item_embedding(), ials.h:410).
  MatrixXf item_embedding() const { return dev_->Get(DeviceContext::ITEM); }
  MatrixXf user_embedding() const { return dev_->Get(DeviceContext::USER); }
  void set_embeddings(const MatrixXf& U, const MatrixXf& V) {
    dev_->Set(DeviceContext::USER, U);
    dev_->Set(DeviceContext::ITEM, V);
    OnEmbeddingsSet();
  }
  const VectorXf& user_loss() const { return user_loss_; }
  // The dual state of ERM-MF / CVaR-MF / SAFER2 (empty for iALS): omega as
  // the last Train() used it, and item_reg_ from Initialize().
  const VectorXf& dual_weights() const { return dual_weight_; }
  const VectorXf& item_regularization() const { return item_reg_; }
  DeviceContext& device() { return *dev_; }

  // ---- checkpoints (frecsys/checkpoint.h) ----
  // The scalar state that lives across Train() calls beside the tables and
  // the three vectors above, as STATE's name=value pairs (checkpoint.h lists
  // the names); RestoreState is false with *err set on a bad value.
  virtual void CaptureState(std::map<std::string, std::string>* kv) { (void)kv; }
  virtual bool RestoreState(const std::map<std::string, std::string>& kv, std::string* err) {
    (void)kv;
    (void)err;
    return true;
  }
  // One table at a time, then TablesSet() once: what set_embeddings does.
  void SetTable(int side, const MatrixXf& m) { dev_->Set(side, m); }
  void TablesSet() { OnEmbeddingsSet(); }
  // The saved vectors (omega / item_reg: nullptr for a model without dual
  // state); with the saved run's tuples also |H_u| (ComputeHistoryStats, whose
  // item_reg_ is then replaced by the saved one: the same values).
  void RestoreVectors(const float* loss, const float* omega, const float* item_reg,
                      const Dataset* data) {
    if (data && omega) ComputeHistoryStats(*data);
    std::memcpy(user_loss_.data(), loss, sizeof(float) * (size_t)user_loss_.size());
    if (omega) std::memcpy(dual_weight_.data(), omega, sizeof(float) * (size_t)dual_weight_.size());
    if (item_reg) std::memcpy(item_reg_.data(), item_reg, sizeof(float) * (size_t)item_reg_.size());
  }

  // The model's projection of held-out users (the fold-in of its
  // EvaluateDataset: ials.h:148-174 and the model variants): row r of `csr`
  // is one user's history; loads it as the EVAL side and leaves the projected
  // embeddings there.
  virtual void FoldIn(const Csr& csr) = 0;

  // The k best items for trained users (rows of U), with scores; exclude_seen
  // drops each user's training history (Train() must have loaded it), mask:
  // [num_items] bytes, non-zero = candidate, or nullptr.  No reference
  // counterpart beyond EvaluateUser's scoring (recommender.h:132-199).
  DeviceContext::Recommendations Recommend(const std::vector<int64_t>& users, int k,
                                           bool exclude_seen, const uint8_t* mask = nullptr) {
    return dev_->Recommend(DeviceContext::USER, users, k,
                           exclude_seen ? FRECSYS_REC_EXCLUDE_HISTORY : 0, mask);
  }
  // The same for unseen users given by their histories: FoldIn, then the
  // ranking of the EVAL rows (exclude_seen drops the fold-in history).
  DeviceContext::Recommendations RecommendFoldIn(const Csr& csr, int k, bool exclude_seen,
                                                 const uint8_t* mask = nullptr) {
    FoldIn(csr);
    std::vector<int64_t> rows((size_t)csr.rows());
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (int64_t)i;
    return dev_->Recommend(DeviceContext::EVAL, rows, k,
                           exclude_seen ? FRECSYS_REC_EXCLUDE_HISTORY : 0, mask);
  }

  // Two-stage lists (frecsys_recommend_two_stage): a bf16 retrieval scan, the
  // pool re-scored exactly, certified[i] = 1 where the list is Recommend's bit
  // for bit (2: re-run exactly, with FRECSYS_TS_EXACT in flags).  Rows, mask
  // and outputs as for RecommendDiverse; certified: host [n] or nullptr.
  int RecommendTwoStage(int side, const int64_t* rows, int64_t n, int k, int pool, int flags,
                        const uint8_t* mask, int32_t* items, float* scores, uint8_t* certified) {
    return frecsys_recommend_two_stage(dev_->raw(), side, rows, n, k, pool, flags, mask, items,
                                       scores, certified, nullptr, nullptr);
  }

  // Diversified lists (frecsys_recommend_diverse): the greedy MMR selection of
  // k from the `pool` best items of each row of `side` (USER: trained users;
  // EVAL: the rows a FoldIn left there), against the model's item table.
  // flags: FRECSYS_REC_EXCLUDE_HISTORY | FRECSYS_DIV_RAW_SCORES; outputs: host
  // [n * k] (mmr may be nullptr).  The status code, for callers that report
  // errors.
  int RecommendDiverse(int side, const int64_t* rows, int64_t n, int k, int pool, float lam,
                       int flags, const uint8_t* mask, int32_t* items, float* scores, float* mmr) {
    return frecsys_recommend_diverse(dev_->raw(), side, rows, n, k, pool, lam, flags, mask, items,
                                     scores, mmr);
  }
  // The same selection from caller-supplied pools, lists / list_scores: host
  // [n * pool] (frecsys_diversify).
  int Diversify(const int32_t* lists, const float* list_scores, int64_t n, int pool, int k,
                float lam, int flags, int32_t* items, float* scores, float* mmr) {
    return frecsys_diversify(dev_->raw(), lists, list_scores, n, pool, k, lam, flags, items, scores,
                             mmr);
  }
  // The DPP selection in the MMR selection's place (frecsys_recommend_dpp,
  // frecsys_diversify_dpp): the same rows, pools, flags and outputs, theta and
  // eps for lam, gain for mmr.
  int RecommendDpp(int side, const int64_t* rows, int64_t n, int k, int pool, float theta,
                   float eps, int flags, const uint8_t* mask, int32_t* items, float* scores,
                   float* gain) {
    return frecsys_recommend_dpp(dev_->raw(), side, rows, n, k, pool, theta, eps, flags, mask,
                                 items, scores, gain);
  }
  int DiversifyDpp(const int32_t* lists, const float* list_scores, int64_t n, int pool, int k,
                   float theta, float eps, int flags, int32_t* items, float* scores, float* gain) {
    return frecsys_diversify_dpp(dev_->raw(), lists, list_scores, n, pool, k, theta, eps, flags,
                                 items, scores, gain);
  }

  // The solve parameters of the model's own fold-in projection -- the ones
  // its FoldIn passes, omega = 1 where the fold-in uses it.  iALS++ and
  // SAFER2++ give the parameters of the objective their block steps descend:
  // their explanation is that of its exact minimiser, which their own fold-in
  // (8 block epochs from zero) only approaches.
  virtual frecsys_solve_params ExplainParams() const = 0;

  // Why an item scores what it does (frecsys_explain): the score of the exact
  // projection of a user's history against the current item table, split over
  // the history entries.  targets: row i holds the targets of users[i] / of
  // history row i; outputs as frecsys_explain's (full may be nullptr).  The
  // status code, for callers that report errors.  Explain needs the training
  // CSR on the device (Train() loads it).
  int Explain(const int64_t* users, int64_t n, const int64_t* tgt_ptr, const int32_t* tgt_items,
              int top, float* score, int32_t* top_items, float* top_contrib, float* full) {
    dev_->Gramian(DeviceContext::ITEM);
    const frecsys_solve_params p = ExplainParams();
    return frecsys_explain(dev_->raw(), DeviceContext::USER, &p, users, n, tgt_ptr, tgt_items, top,
                           score, top_items, top_contrib, full);
  }
  // The same for unseen users given by their histories, loaded as the EVAL side.
  int ExplainFoldIn(const Csr& csr, const int64_t* tgt_ptr, const int32_t* tgt_items, int top,
                    float* score, int32_t* top_items, float* top_contrib, float* full) {
    dev_->LoadEval(csr);
    dev_->Gramian(DeviceContext::ITEM);
    const frecsys_solve_params p = ExplainParams();
    return frecsys_explain(dev_->raw(), DeviceContext::EVAL, &p, nullptr, csr.rows(), tgt_ptr,
                           tgt_items, top, score, top_items, top_contrib, full);
  }

  // Ranking quality of trained users on the device (frecsys_rank_metrics):
  // row i of `gt` is the ground truth of users[i]; Recall@K / NDCG@K of
  // Recommend's ranking at every cut-off of k_list, per user, in the
  // reference's EvaluationResult (show() prints its lines; cvar() its tail
  // means).  Only the users x |k_list| metric rows leave the device.
  EvaluationResult Evaluate(const std::vector<int64_t>& users, const Csr& gt,
                            const VectorXi& k_list, const VectorXf& alpha_list,
                            bool exclude_seen) {
    return RankMetricsOf(DeviceContext::USER, users, gt, k_list, alpha_list, exclude_seen);
  }
  // The same for unseen users given by their histories: FoldIn, then the
  // metrics of the EVAL rows (row i of `gt` belongs to row i of `csr`).  The
  // projected rows stay in the EVAL side, as with RecommendFoldIn.
  EvaluationResult EvaluateFoldIn(const Csr& csr, const Csr& gt, const VectorXi& k_list,
                                  const VectorXf& alpha_list, bool exclude_seen) {
    FoldIn(csr);
    std::vector<int64_t> rows((size_t)csr.rows());
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (int64_t)i;
    return RankMetricsOf(DeviceContext::EVAL, rows, gt, k_list, alpha_list, exclude_seen);
  }

 protected:
  EvaluationResult RankMetricsOf(int side, const std::vector<int64_t>& rows, const Csr& gt,
                                 const VectorXi& k_list, const VectorXf& alpha_list,
                                 bool exclude_seen) {
    std::vector<int32_t> ks((size_t)k_list.size());
    for (size_t i = 0; i < ks.size(); ++i) ks[i] = k_list[(int64_t)i];
    DeviceContext::Metrics m = dev_->RankMetrics(
        side, rows, exclude_seen ? FRECSYS_REC_EXCLUDE_HISTORY : 0, gt, ks);
    return EvaluationResult{k_list, alpha_list, std::move(m.recall), std::move(m.ndcg)};
  }

  virtual void OnEmbeddingsSet() {}

  // STATE values (checkpoint.h): a float travels as its bit pattern.
  static std::string FloatBits(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return std::to_string(b);
  }
  // The u64 / float named `name`; false with *err set when absent or malformed.
  static bool StateU64(const std::map<std::string, std::string>& kv, const char* name,
                       uint64_t max, uint64_t* v, std::string* err) {
    const auto it = kv.find(name);
    char* e = nullptr;
    errno = 0;
    const unsigned long long x =
        it == kv.end() || it->second.empty() || it->second[0] == '-' ? 0
                                                                     : strtoull(it->second.c_str(), &e, 10);
    if (!e || *e || errno || x > max) {
      *err = std::string(name) + " is missing or malformed";
      return false;
    }
    *v = x;
    return true;
  }
  static bool StateFloatBits(const std::map<std::string, std::string>& kv, const char* name,
                             float* x, std::string* err) {
    uint64_t b;
    if (!StateU64(kv, name, UINT32_MAX, &b, err)) return false;
    const uint32_t b32 = (uint32_t)b;
    std::memcpy(x, &b32, 4);
    return true;
  }

  // FoldIn of the models that project with one solve (ials.h:148-185 and its
  // variants): the EVAL rows solved with `params`.
  void FoldInSolve(const Csr& csr, const frecsys_solve_params& params) {
    dev_->LoadEval(csr);
    dev_->Solve(DeviceContext::EVAL, params);
  }

  // Fold-in + evaluation (then EvaluateDatasetInternal / EvaluateUser,
  // recommender.h:78-199): project the users of `data` (FoldIn), score every
  // item, exclude each user's fold-in history and rank -- all on the GPU
  // (frecsys_eval_topk); Recall / NDCG of the k_list cut-offs on host.
  EvaluationResult FoldInEvaluate(const VectorXi& k_list, const VectorXf& alpha_list,
                                  const Dataset& data, const SpMatrix& eval_by_user) {
    std::vector<int32_t> ids;
    Csr csr;
    data.compact_users(&ids, &csr);
    FoldIn(csr);
    return RankEval(k_list, alpha_list, ids, eval_by_user);
  }

  // Ranking of the projected EVAL rows (ids = their user ids): GPU scoring +
  // top-K, Recall / NDCG on host (recommender.h:132-199).
  EvaluationResult RankEval(const VectorXi& k_list, const VectorXf& alpha_list,
                            const std::vector<int32_t>& ids, const SpMatrix& eval_by_user) {
    const int max_k = std::min<int>(k_list.maxCoeff(), (int)num_items_);
    const std::vector<int32_t> top = dev_->EvalTopK(max_k);
    std::unordered_map<int, int> user_to_ind;
    for (size_t i = 0; i < ids.size(); ++i) user_to_ind[ids[i]] = (int)i;
    const int64_t nk = k_list.size();
    const int64_t nu = (int64_t)eval_by_user.size();
    MatrixXf recall = MatrixXf::Zero(nu, nk), ndcg = MatrixXf::Zero(nu, nk);
    int row = 0;
    for (const auto& kv : eval_by_user) {
      const int32_t* t = top.data() + (size_t)user_to_ind.at(kv.first) * max_k;
      const UserEvaluationResult m = RankMetrics(k_list, t, max_k, kv.second);
      for (int64_t i = 0; i < nk; ++i) {
        recall(row, i) = m.recall[i];
        ndcg(row, i) = m.ndcg[i];
      }
      ++row;
    }
    return EvaluationResult{k_list, alpha_list, recall, ndcg};
  }

  // Initialize() bookkeeping of ERM-MF / CVaR-MF / SAFER2
  // (safer2.h:827-837): |H_u| and item_reg_[v] = sum_{u in H_v} 1/|H_u|
  // accumulated in by_item (file) order.
  void ComputeHistoryStats(const Dataset& data) {
    user_history_size_ = VectorXf::Zero(num_users_);
    item_reg_ = VectorXf::Zero(num_items_);
    const Csr& u = data.user_csr();
    const Csr& it = data.item_csr();
    for (int64_t r = 0; r < u.rows() && r < num_users_; ++r) user_history_size_[r] = (float)u.len(r);
    for (int64_t v = 0; v < it.rows() && v < num_items_; ++v)
      for (int64_t k = it.ptr[v]; k < it.ptr[v + 1]; ++k)
        item_reg_[v] = (float)((double)item_reg_[v] + 1.0 / (double)user_history_size_[it.col[k]]);
  }

  // VaR / CVaR of the user losses (safer2.h:304-316).
  void PrintVarStats(float alpha) const {
    std::vector<float> vals((size_t)user_loss_.size());
    for (int64_t i = 0; i < user_loss_.size(); ++i) vals[i] = -user_loss_[i];
    const size_t Q = (size_t)((float)vals.size() * alpha);
    std::nth_element(vals.begin(), vals.begin() + Q, vals.end());
    float loss = 0;
    for (size_t i = 0; i <= Q; i++) loss += -vals[i];
    LOG(INFO) << "VaR: " << -vals[Q] << " CVaR: " << loss / (float)Q;
  }

  // Train-loss diagnostics (ials.h:226-305, safer2.h:337-413): the
  // observed / unobserved sums and the squared row norms of U and V, computed
  // on the GPU (frecsys_train_stats); counted in Train() time like the
  // reference's (run_model flag --print_train_stats, default on).
  struct LossParts {
    double observed = 0, unobserved = 0;
    std::vector<float> user_norm2, item_norm2;
  };
  LossParts ComputeLossParts(const Dataset& data) {
    (void)data;
    LossParts lp;
    lp.user_norm2.resize((size_t)num_users_);
    lp.item_norm2.resize((size_t)num_items_);
    dev_->TrainStats(&lp.observed, &lp.unobserved, lp.user_norm2.data(), lp.item_norm2.data());
    return lp;
  }

  // PrintLosses of the weighted models (safer2.h:337-413, erm_mf.h:303-377,
  // cvar_mf.h:332-406 -- identical): loss = sum of the user losses, the
  // regularisers with UserRegularizationValue / ItemRegularizationValue.
  void PrintWeightedLosses(const Dataset& data, float reg, float w, float alpha) {
    if (!print_trainstats_) return;
    const auto t0 = std::chrono::steady_clock::now();
    const LossParts lp = ComputeLossParts(data);
    const Csr& uc = data.user_csr();
    const Csr& ic = data.item_csr();
    float loss_reg = 0.0f, reg_user_now = 0.0f, reg_item_now = 0.0f;
    for (int64_t u = 0; u < uc.rows(); ++u) {
      if (!uc.len(u)) continue;
      const float n2 = lp.user_norm2[u];
      loss_reg += n2 * (reg * (1 + w * num_items_));
      reg_user_now += n2;
    }
    for (int64_t i = 0; i < ic.rows(); ++i) {
      if (!ic.len(i)) continue;
      const float n2 = lp.item_norm2[i];
      loss_reg += n2 * (reg * (item_reg_[i] + alpha * w * num_users_));
      reg_item_now += n2;
    }
    const float loss = user_loss_.sum();
    const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                        std::chrono::steady_clock::now() - t0)
                        .count();
    CheckNaN(loss);
    LOG(INFO) << format(
        "Loss={0:.2f} Loss_observed={1:.2f} Loss_unobserved={2:.2f} Loss_reg={3:.2f} "
        "Loss_reg (user)={4:.2f} Loss_reg (item)={5:.2f}",
        loss, lp.observed / data.num_tuples(), lp.unobserved / num_items_ / num_users_, loss_reg,
        reg_user_now / num_users_, reg_item_now / num_items_);
    LOG(INFO) << format("Time={0}", (int64_t)ms);
  }

  // (w - w_prev).norm() of the dual weights (ComputeUserWeights' residual,
  // safer2.h:789-792, cvar_mf.h:637-640), in double.
  static float WeightResidual(const VectorXf& w, const VectorXf& prev) {
    double s = 0.0;
    for (int64_t i = 0; i < w.size(); ++i) {
      const double d = (double)w[i] - (double)prev[i];
      s += d * d;
    }
    return (float)std::sqrt(s);
  }

  static double RowSqNorm(const MatrixXf& M, int64_t r) {
    double s = 0;
    for (int64_t j = 0; j < M.cols(); ++j) s += (double)M(r, j) * M(r, j);
    return s;
  }

  void CheckNaN(float loss) const {
    if (std::isnan(loss)) {  // ials.h:291-296: logged, then exit(0)
      LOG(ERROR) << "!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!";
      LOG(ERROR) << "NaN is detected!!";
      LOG(ERROR) << "!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!!";
      std::exit(0);
    }
  }

  int dim_;
  int64_t num_users_, num_items_;
  DeviceOptions opts_;
  std::unique_ptr<DeviceContext> dev_;
  VectorXf user_loss_;
  VectorXf dual_weight_;
  VectorXf user_history_size_;
  VectorXf item_reg_;
  bool print_trainstats_ = false;
  bool print_residualstats_ = false;  // uninitialised in the reference
  bool print_varstats_ = false;
};

inline void check_ok(int rc) {
  if (rc != FRECSYS_OK) LOG(FATAL) << "frecsys call failed (" << rc << "): " << frecsys_last_error(nullptr);
}

// One-entity projection through a temporary device context: the reference's
// static Project / ProjectU / ProjectV (ials.h:88, safer2.h:104, 166) with
// `reg` used as the final lambda.
inline VectorXf ProjectOnDevice(int kind, const SpVector& history, const MatrixXf& X,
                                const MatrixXf& G, float reg, float w, float weight,
                                const VectorXf* nu, bool use_cg = false,
                                float cg_error_tolerance = 1e-10f, int cg_max_iterations = 100) {
  const int d = (int)X.cols();
  DeviceOptions o;
  o.world = 1;
  o.rank = 0;
  DeviceContext ctx(d, 1, X.rows(), o);
  ctx.SetCg(use_cg, cg_error_tolerance, cg_max_iterations);
  Csr c;
  c.ptr = {0, (int64_t)history.size()};
  for (const auto& p : history) c.col.push_back(p.first);
  // side USER (1 row) against ITEM = X
  check_ok(frecsys_load_csr(ctx.raw(), FRECSYS_SIDE_USER, 1, c.ptr.data(), c.col.data()));
  ctx.Set(DeviceContext::ITEM, X);
  check_ok(frecsys_set_gramian(ctx.raw(), FRECSYS_SIDE_ITEM, G.data(), d));
  frecsys_solve_params p = solve_params(kind, reg, w);
  p.lambda_is_reg = 1;
  float om = weight;
  std::vector<float> er(1, 0.0f);
  std::vector<float> nuv;
  if (kind == FRECSYS_KIND_WEIGHTED_U) p.entity_weight = &om;
  if (kind == FRECSYS_KIND_WEIGHTED_V) {
    nuv.assign(nu->data(), nu->data() + nu->size());
    p.entity_reg = er.data();
    p.other_weight = nuv.data();
  }
  ctx.Solve(DeviceContext::USER, p);
  MatrixXf out = ctx.Get(DeviceContext::USER);
  VectorXf x(d);
  for (int j = 0; j < d; ++j) x[j] = out(0, j);
  return x;
}

}  // namespace detail
}  // namespace frecsys
