// model_capi.cc -- libfrecsys_model.so, the C-ABI of include/frecsys_model.h
// over the C++ model classes (include/frecsys/*.h).  A thin owner of one
// Dataset + one Recommender built by the run_model factory
// (frecsys/factory.h); every compute call lands in libfrecsys_hip.so.
//
// The query entry points (recommend, rank_candidates, the evaluations, explain,
// recommend_diverse) come as a trained-users form and a _fold_in form.  Each
// pair is one function over a Query -- trained user ids or a history CSR --
// that open_query() checks and, for histories, projects; the extern "C"
// functions only name the call and build the Query.  The stored model flags
// are listed once, in checkpoint.h (ForEachConfigField).
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "frecsys/checkpoint.h"
#include "frecsys/factory.h"
#include "frecsys_model.h"

struct frecsys_model {
  std::string name;
  frecsys::checkpoint::Config config;       // what a checkpoint's CONFIG holds
  std::unique_ptr<frecsys::Dataset> train;  // null: loaded without tuples (serve-only)
  std::unique_ptr<frecsys::Recommender> rec;
  int64_t epochs = 0;            // Train() calls so far, a loaded model's included
  bool restored = false;         // loaded in its saved state: already initialised
  int64_t n_tuples = 0;          // of a loaded model's file, for a save without a dataset
  uint64_t tuples_checksum = 0;
};

namespace {
namespace ck = frecsys::checkpoint;

std::string g_model_error;
int model_fail(int code, const std::string& msg) {
  g_model_error = msg;
  return code;
}
}  // namespace

extern "C" {

void frecsys_model_config_default(frecsys_model_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));  // world 0, comm_id and model_name null
  ck::CopyConfigFields(frecsys::ModelParams(), c);  // run_model.cc:129-230 defaults
  c->seed = -1;
  c->device = -1;
  c->parity_quirks = 1;
  c->rank = -1;
}

}  // extern "C"

namespace {

// The stored fields of a C config (device / world / rank / comm_id stay out),
// the flags among them as 0 / 1: through ModelParams, where they are bools.
ck::Config stored_config(const frecsys_model_config& c, const std::string& name) {
  frecsys::ModelParams p;
  ck::CopyConfigFields(c, &p);
  return ck::FromParams(name, p, c.seed, c.parity_quirks != 0);
}
// ... and back, on top of the defaults; model_name is left to the caller.
void c_config(const ck::Config& k, frecsys_model_config* c) {
  frecsys_model_config_default(c);
  ck::CopyConfigFields(k, c);
}

// The use_cg and block_size rules of a configuration, which need no device
// (conditions the C++ constructors treat as fatal); FRECSYS_OK when fine.
int config_check(const frecsys_model_config* c, const std::string& name) {
  const bool cg_model = name == "ials" || name == "safer2";
  if ((name == "ialspp" || name == "safer2pp") && (c->block_size < 1 || c->block_size > 128))
    return model_fail(FRECSYS_ERR_INVALID, "block_size must be in [1, 128] (got " +
                                               std::to_string(c->block_size) + ")");
  if (c->use_cg && name == "erm_mf")  // fatal in the C++ constructor; before any device call
    return model_fail(FRECSYS_ERR_UNSUPPORTED,
                      "erm_mf: use_cg is not supported (the reference's BiCGSTAB path, "
                      "erm_mf.h:103-145, is not built)");
  if (c->use_cg && cg_model &&
      (c->cg_max_iterations < 0 || !(c->cg_error_tolerance >= 0.0f)))
    return model_fail(FRECSYS_ERR_INVALID,
                      "cg_max_iterations and cg_error_tolerance must be >= 0 (and not NaN)");
  if (c->use_cg && cg_model && c->dim > 256)
    return model_fail(FRECSYS_ERR_UNSUPPORTED,
                      "use_cg: the conjugate-gradient path is built for dim <= 256");
  return FRECSYS_OK;
}

int device_check() {
  int32_t ndev = 0;  // the C++ layer aborts on a missing device; report it instead
  if (frecsys_device_count(&ndev) != FRECSYS_OK || ndev == 0)
    return model_fail(FRECSYS_ERR_NO_DEVICE, "no HIP device visible");
  return FRECSYS_OK;
}

// The model of a checked configuration, sized n_users x n_items, with its
// dataset (nullptr: a serve-only model).
std::unique_ptr<frecsys_model> make_model(const frecsys_model_config* c, const std::string& name,
                                          int64_t n_users, int64_t n_items,
                                          std::unique_ptr<frecsys::Dataset> train) {
  frecsys::DeviceOptions o;
  o.seed = c->seed;
  o.device = c->device;
  o.parity_quirks = c->parity_quirks != 0;
  o.world = c->world;
  o.rank = c->rank;
  if (c->comm_id) {
    o.has_comm_id = true;
    std::memcpy(o.comm_id.data(), c->comm_id, 128);
  }
  auto m = std::make_unique<frecsys_model>();
  m->name = name;
  m->config = stored_config(*c, name);
  m->train = std::move(train);
  m->rec.reset(frecsys::MakeRecommender(name, (int)n_users, (int)n_items, ck::ToParams(m->config), o));
  return m;
}

// exclude_seen / Train() need the training tuples: a model loaded without
// them answers with an error instead of reaching the C++ layer, where a
// failed device call is fatal.
int needs_data(const frecsys_model* m, const char* what) {
  if (m->train) return FRECSYS_OK;
  return model_fail(FRECSYS_ERR_INVALID,
                    std::string(what) + ": the model was loaded without training tuples "
                                        "(serve-only): no training and no exclude_seen");
}

}  // namespace

extern "C" {

int frecsys_model_create(const frecsys_model_config* c, const int32_t* users, const int32_t* items,
                         int64_t n_tuples, frecsys_model** out) {
  if (!c || !out || n_tuples <= 0 || !users || !items || !c->model_name)
    return model_fail(FRECSYS_ERR_INVALID, "frecsys_model_create: bad arguments");
  *out = nullptr;
  const std::string name = c->model_name;
  if (!frecsys::IsKnownModel(name))
    return model_fail(FRECSYS_ERR_INVALID, "unknown model " + name);
  if (frecsys_padded_dim(c->dim) == 0)
    return model_fail(FRECSYS_ERR_UNSUPPORTED, "dim " + std::to_string(c->dim) + " not built");
  for (int64_t k = 0; k < n_tuples; ++k)
    if (users[k] < 0 || items[k] < 0)
      return model_fail(FRECSYS_ERR_INVALID, "negative id in tuple " + std::to_string(k));
  if (int rc = config_check(c, name)) return rc;
  if (int rc = device_check()) return rc;
  auto train = std::make_unique<frecsys::Dataset>(std::vector<int32_t>(users, users + n_tuples),
                                                  std::vector<int32_t>(items, items + n_tuples));
  const int64_t nu = train->max_user() + 1, ni = train->max_item() + 1;
  *out = make_model(c, name, nu, ni, std::move(train)).release();
  return FRECSYS_OK;
}

int frecsys_model_initialize(frecsys_model* m) {
  if (!m) return model_fail(FRECSYS_ERR_INVALID, "null model");
  if (m->restored) return FRECSYS_OK;  // a loaded model comes back initialised
  if (int rc = needs_data(m, "frecsys_model_initialize")) return rc;
  frecsys::InitializeRecommender(m->name, m->rec.get(), *m->train);
  return FRECSYS_OK;
}

int frecsys_model_train(frecsys_model* m, int32_t epochs) {
  if (!m || epochs < 0) return model_fail(FRECSYS_ERR_INVALID, "frecsys_model_train: bad arguments");
  if (int rc = needs_data(m, "frecsys_model_train")) return rc;
  for (int32_t e = 0; e < epochs; ++e) {
    m->rec->Train(*m->train);
    ++m->epochs;
  }
  return FRECSYS_OK;
}

int64_t frecsys_model_epochs(const frecsys_model* m) { return m ? m->epochs : -1; }

int frecsys_model_save(frecsys_model* m, const char* path, int32_t flags) {
  if (!m || !path || !*path || (flags & ~FRECSYS_SAVE_NO_DATA))
    return model_fail(FRECSYS_ERR_INVALID, "frecsys_model_save: bad arguments");
  ck::Tuples t;
  t.n = m->n_tuples;
  t.checksum = m->tuples_checksum;
  if (m->train) {
    t.n = m->train->num_tuples();
    t.checksum = ck::TuplesChecksum(m->train->users().data(), m->train->items().data(), t.n);
    if (!(flags & FRECSYS_SAVE_NO_DATA)) {
      t.users = m->train->users().data();
      t.items = m->train->items().data();
    }
  }
  std::string err;
  const ck::Status s = ck::SaveModel(m->config, frecsys::AsDeviceModel(m->rec.get()), t, m->epochs,
                                     path, &err);
  return s == ck::kOk ? FRECSYS_OK : model_fail((int)s, "frecsys_model_save: " + err);
}

int frecsys_model_file_info(const char* path, int32_t verify, frecsys_model_file_info_t* info) {
  if (!path || !info) return model_fail(FRECSYS_ERR_INVALID, "frecsys_model_file_info: bad arguments");
  ck::Reader r;
  std::string err;
  const ck::Status s = r.Open(path, verify != 0, &err);
  if (s != ck::kOk) return model_fail((int)s, err);
  const ck::Info& in = r.info();
  std::memset(info, 0, sizeof(*info));
  snprintf(info->model_name, sizeof(info->model_name), "%s", in.config.model_name.c_str());
  c_config(in.config, &info->config);
  info->config.model_name = info->model_name;
  info->n_users = in.n_users;
  info->n_items = in.n_items;
  info->n_tuples = in.n_tuples;
  info->epochs_trained = in.epochs_trained;
  info->flags = in.flags;
  info->tuples_checksum = in.tuples_checksum;
  info->version = in.version;
  return FRECSYS_OK;
}

int frecsys_model_load(const char* path, const frecsys_model_config* cfg, const int32_t* users,
                       const int32_t* items, int64_t n_tuples, int32_t flags,
                       frecsys_model** out) {
  const std::string w = "frecsys_model_load: ";
  if (!path || !out || (flags & ~FRECSYS_LOAD_TABLES_ONLY) || (users != nullptr) != (items != nullptr) ||
      (users && n_tuples <= 0))
    return model_fail(FRECSYS_ERR_INVALID, w + "bad arguments");
  *out = nullptr;
  const bool tables_only = (flags & FRECSYS_LOAD_TABLES_ONLY) != 0;
  // the whole file is validated before the first device call
  ck::Reader r;
  std::string err;
  ck::Status s = r.Open(path, true, &err);
  if (s != ck::kOk) return model_fail((int)s, w + err);
  const ck::Info& in = r.info();
  frecsys_model_config c;
  const std::string name = in.config.model_name;
  if (cfg) {
    c = *cfg;
    if (!c.model_name || name != c.model_name)
      return model_fail(FRECSYS_ERR_INVALID, w + "model_name differs from the file's (" + name + ")");
    if (c.dim != in.config.dim)
      return model_fail(FRECSYS_ERR_INVALID, w + "dim " + std::to_string(c.dim) +
                                                 " differs from the file's (" +
                                                 std::to_string(in.config.dim) + ")");
    if (!tables_only && (c.parity_quirks != 0) != (in.config.parity_quirks != 0))
      return model_fail(FRECSYS_ERR_INVALID, w + "parity_quirks differs from the file's");
  } else {
    c_config(in.config, &c);
  }
  c.model_name = name.c_str();
  if (int rc = config_check(&c, name)) return rc;

  std::unique_ptr<frecsys::Dataset> train;
  int64_t nu = in.n_users, ni = in.n_items;
  if (users) {
    int32_t mu = -1, mi = -1;
    for (int64_t k = 0; k < n_tuples; ++k) {
      if (users[k] < 0 || items[k] < 0)
        return model_fail(FRECSYS_ERR_INVALID, w + "negative id in tuple " + std::to_string(k));
      mu = std::max(mu, users[k]);
      mi = std::max(mi, items[k]);
    }
    if (tables_only) {
      if (mu + 1 < in.n_users || mi + 1 < in.n_items)
        return model_fail(FRECSYS_ERR_INVALID,
                          w + "the tuples span fewer users or items than the stored tables hold");
      nu = (int64_t)mu + 1;
      ni = (int64_t)mi + 1;
    } else {
      if (n_tuples != in.n_tuples)
        return model_fail(FRECSYS_ERR_INVALID,
                          w + "the tuples passed are not the saved run's: " + std::to_string(n_tuples) +
                              " tuples, the file was written for " + std::to_string(in.n_tuples));
      if (ck::TuplesChecksum(users, items, n_tuples) != in.tuples_checksum || mu >= in.n_users ||
          mi >= in.n_items)
        return model_fail(FRECSYS_ERR_INVALID,
                          w + "the tuples passed are not the saved run's: their checksum differs "
                              "from the file's tuples_checksum (other ids or another order)");
    }
    train = std::make_unique<frecsys::Dataset>(std::vector<int32_t>(users, users + n_tuples),
                                               std::vector<int32_t>(items, items + n_tuples));
  } else if (tables_only) {
    return model_fail(FRECSYS_ERR_INVALID, w + "FRECSYS_LOAD_TABLES_ONLY needs the caller's tuples");
  } else if (r.has_tuples()) {
    std::vector<int32_t> u((size_t)in.n_tuples), it((size_t)in.n_tuples);
    if ((s = r.Read("USERS", u.data(), u.size() * 4, &err)) != ck::kOk ||
        (s = r.Read("ITEMS", it.data(), it.size() * 4, &err)) != ck::kOk)
      return model_fail((int)s, w + err);
    // read a second time after the verification pass: checked again
    if (ck::TuplesChecksum(u.data(), it.data(), in.n_tuples) != in.tuples_checksum)
      return model_fail(FRECSYS_ERR_INVALID, w + "the file changed while it was read");
    for (int64_t k = 0; k < in.n_tuples; ++k)
      if (u[k] < 0 || u[k] >= in.n_users || it[k] < 0 || it[k] >= in.n_items)
        return model_fail(FRECSYS_ERR_INVALID, w + "the file changed while it was read");
    train = std::make_unique<frecsys::Dataset>(std::move(u), std::move(it));
  }
  if (int rc = device_check()) return rc;

  auto m = make_model(&c, name, nu, ni, std::move(train));
  frecsys::detail::DeviceModel* dm = frecsys::AsDeviceModel(m->rec.get());
  if (tables_only) {
    s = ck::RestoreTables(r, dm, &err);
  } else {
    s = ck::RestoreModel(r, dm, m->train.get(), &err);
    m->restored = true;
    m->epochs = in.epochs_trained;
    m->n_tuples = in.n_tuples;
    m->tuples_checksum = in.tuples_checksum;
  }
  if (s != ck::kOk) return model_fail((int)s, w + err);
  *out = m.release();
  return FRECSYS_OK;
}

frecsys_ctx* frecsys_model_context(frecsys_model* m) {
  return m ? frecsys::AsDeviceModel(m->rec.get())->device().raw() : nullptr;
}

float frecsys_model_mean_weight(const frecsys_model* m) {
  if (!m) return NAN;
  frecsys::Recommender* r = m->rec.get();
  if (m->name == "safer2" || m->name == "safer2pp")
    return static_cast<frecsys::SAFER2Recommender*>(r)->GetMeanWeight();
  if (m->name == "erm_mf") return static_cast<frecsys::ERMMFRecommender*>(r)->GetMeanWeight();
  if (m->name == "cvar_mf") return static_cast<frecsys::CVaRMFRecommender*>(r)->GetMeanWeight();
  return NAN;
}

int frecsys_model_dual_state(const frecsys_model* m, float* weights, float* losses,
                             float* item_reg, float* xi) {
  if (!m) return model_fail(FRECSYS_ERR_INVALID, "null model");
  const frecsys::detail::DeviceModel* dm = frecsys::AsDeviceModel(m->rec.get());
  const frecsys::VectorXf& w = dm->dual_weights();
  if ((weights || item_reg) && w.size() == 0)
    return model_fail(FRECSYS_ERR_INVALID, m->name + " has no dual weights");
  if (weights) std::memcpy(weights, w.data(), sizeof(float) * (size_t)w.size());
  if (losses) {
    const frecsys::VectorXf& l = dm->user_loss();
    std::memcpy(losses, l.data(), sizeof(float) * (size_t)l.size());
  }
  if (item_reg) {
    const frecsys::VectorXf& r = dm->item_regularization();
    std::memcpy(item_reg, r.data(), sizeof(float) * (size_t)r.size());
  }
  if (xi) {
    *xi = NAN;
    if (m->name == "safer2" || m->name == "safer2pp")
      *xi = static_cast<const frecsys::SAFER2Recommender*>(m->rec.get())->xi();
  }
  return FRECSYS_OK;
}

}  // extern "C"

namespace {

using frecsys::DeviceContext;

// The status of a context call: the context's message goes with its code.
int context_status(DeviceContext& dev, int rc) {
  return rc ? model_fail(rc, frecsys_last_error(dev.raw())) : FRECSYS_OK;
}

int exclude_flag(int32_t exclude_seen) { return exclude_seen ? FRECSYS_REC_EXCLUDE_HISTORY : 0; }

// ---- argument checks, before any device call (the C++ layer treats a failed
// device call and a bad EVAL CSR as fatal); "" when fine ----

std::string hist_args_error(int64_t n, int64_t n_items, const int64_t* hist_ptr,
                            const int32_t* hist_items) {
  if (n < 0 || !hist_ptr || hist_ptr[0] != 0) return "bad arguments";
  for (int64_t i = 0; i < n; ++i)
    if (hist_ptr[i + 1] < hist_ptr[i]) return "hist_ptr not monotone";
  if (hist_ptr[n] > 0 && !hist_items) return "null hist_items";
  for (int64_t p = 0; p < hist_ptr[n]; ++p)
    if (hist_items[p] < 0 || hist_items[p] >= n_items)
      return "item id " + std::to_string(hist_items[p]) + " out of range";
  return "";
}

std::string cand_args_error(int64_t n, int64_t n_items, const int64_t* cand_ptr,
                            const int32_t* cand_items) {
  if (!cand_ptr || cand_ptr[0] != 0) return "bad cand_ptr";
  for (int64_t i = 0; i < n; ++i)
    if (cand_ptr[i + 1] < cand_ptr[i]) return "cand_ptr not monotone";
  if (cand_ptr[n] > 0 && !cand_items) return "null cand_items";
  for (int64_t p = 0; p < cand_ptr[n]; ++p)
    if (cand_items[p] < 0 || cand_items[p] >= n_items)
      return "candidate id " + std::to_string(cand_items[p]) + " out of range";
  return "";
}

std::string k_items_error(int32_t k, int64_t n, const int32_t* items) {
  return k < 1 || k > 1024 || (n > 0 && !items) ? "k must be in [1, 1024], items non-null" : "";
}

// The pieces of the evaluations' checks: the row count and the head of the
// ground-truth CSR, the alphas, and the CSR's rows and ids (gt_items not null
// when there are rows: the caller's check).
std::string truth_head_error(int64_t n, const int64_t* gt_ptr) {
  return n < 0 || !gt_ptr || gt_ptr[0] != 0 ? "bad arguments (n < 0, gt_ptr)" : "";
}
std::string alpha_error(const float* alpha_list, int32_t na) {
  return na < 0 || (na > 0 && !alpha_list) ? "bad alpha_list" : "";
}
std::string truth_rows_error(int64_t n, int64_t n_items, const int64_t* gt_ptr,
                             const int32_t* gt_items) {
  for (int64_t i = 0; i < n; ++i)
    if (gt_ptr[i + 1] <= gt_ptr[i])
      return "gt_ptr not monotone or no ground truth at row " + std::to_string(i);
  for (int64_t p = 0; p < gt_ptr[n]; ++p)
    if (gt_items[p] < 0 || gt_items[p] >= n_items)
      return "ground-truth id " + std::to_string(gt_items[p]) + " out of range";
  return "";
}

// The arguments every Recall / NDCG evaluation shares.
struct Metrics {
  const int64_t* gt_ptr;
  const int32_t* gt_items;
  const int32_t* k_list;
  int32_t nk;
  const float* alpha_list;
  int32_t na;
  float* recall;
  float* ndcg;
  float* summary;
};

std::string metrics_args_error(int64_t n, int64_t n_items, const Metrics& mt) {
  std::string e = truth_head_error(n, mt.gt_ptr);
  if (!e.empty()) return e;
  if (!mt.k_list || mt.nk < 1 || mt.nk > 32) return "k_list must hold 1 to 32 cut-offs";
  for (int32_t q = 0; q < mt.nk; ++q)
    if (mt.k_list[q] < 1 || mt.k_list[q] > 1024) return "cut-offs must be in [1, 1024]";
  if (!(e = alpha_error(mt.alpha_list, mt.na)).empty()) return e;
  if (n > 0 && (!mt.recall || !mt.ndcg || !mt.gt_items)) return "null gt_items / recall / ndcg";
  return truth_rows_error(n, n_items, mt.gt_ptr, mt.gt_items);
}

// The cases the MMR calls reject (frecsys_hip.h).
std::string diverse_args_error(int32_t k, int32_t pool, float lam, int32_t raw_scores, int64_t n,
                               const int32_t* items, const float* scores) {
  if (pool < 1 || pool > 1024) return "pool must be in [1, 1024]";
  if (k < 1 || k > pool) return "k must be in [1, pool]";
  if (!(lam >= 0.0f && lam <= 1.0f)) return "lam must be in [0, 1]";
  if (raw_scores != 0 && raw_scores != 1) return "raw_scores must be 0 or 1";
  if (n > 0 && (!items || !scores)) return "null outputs";
  return "";
}

// The cases the DPP calls reject (frecsys_hip.h): the MMR calls' with theta
// and eps in lam's place.
std::string dpp_args_error(int32_t k, int32_t pool, float theta, float eps, int32_t raw_scores,
                           int64_t n, const int32_t* items, const float* scores) {
  if (pool < 1 || pool > 1024) return "pool must be in [1, 1024]";
  if (k < 1 || k > pool) return "k must be in [1, pool]";
  if (!(theta >= 0.0f && std::isfinite(theta))) return "theta must be finite and >= 0";
  if (!(eps > 0.0f && eps <= 1.0f)) return "eps must be in (0, 1]";
  if (raw_scores != 0 && raw_scores != 1) return "raw_scores must be 0 or 1";
  if (n > 0 && (!items || !scores)) return "null outputs";
  return "";
}

int32_t diverse_flags(int32_t exclude_seen, int32_t raw_scores) {
  return exclude_flag(exclude_seen) | (raw_scores ? FRECSYS_DIV_RAW_SCORES : 0);
}

// ---- the query rows of a model call ----

// n trained users (rows of U), or the histories of n unseen users as a CSR,
// which the model projects into the EVAL side of its context.
struct Query {
  const int64_t* users;
  const int64_t* hist_ptr;
  const int32_t* hist_items;
  int64_t n;
  bool fold_in;
};
Query trained(const int64_t* users, int64_t n) { return {users, nullptr, nullptr, n, false}; }
Query unseen(const int64_t* hist_ptr, const int32_t* hist_items, int64_t n) {
  return {nullptr, hist_ptr, hist_items, n, true};
}

// Where an opened query's rows are: the side and the row ids to hand to the
// context (nullptr: rows 0 .. n-1, the projected ones).
struct Rows {
  frecsys::detail::DeviceModel* dm = nullptr;
  int side = FRECSYS_SIDE_USER;
  const int64_t* ids = nullptr;
  DeviceContext& dev() const { return dm->device(); }
};

// open_query's answer for zero histories: nothing to project, nothing to run.
// Not a status code; the entry point answers (answered() for most).  Zero
// trained users go on to the context, which answers for them.
constexpr int kNoRows = -1;
int answered(int rc) { return rc == kNoRows ? FRECSYS_OK : rc; }

// What every query entry point does first, in this order: the model; the
// training tuples where the call reads them (exclude_seen on trained users);
// the history CSR; the entry point's own checks, own_error(n_items); the
// trained rows (last: the evaluations word a negative n themselves); then,
// with every check done, the projection of the histories -- the model's
// FoldIn, or for explain the bare LoadEval.  `w` is the prefix of every
// message, "<entry point>: ".
enum Projection { kFoldIn, kLoadOnly };
template <class OwnError>
int open_query(frecsys_model* m, const std::string& w, const Query& q, int32_t reads_training,
               OwnError own_error, Rows* r, Projection projection = kFoldIn) {
  if (!m) return model_fail(FRECSYS_ERR_INVALID, w + "bad arguments");
  if (reads_training && !q.fold_in)
    if (int rc = needs_data(m, w.substr(0, w.size() - 2).c_str())) return rc;
  r->dm = frecsys::AsDeviceModel(m->rec.get());
  const int64_t n_items = r->dev().rows(DeviceContext::ITEM);
  std::string e = q.fold_in ? hist_args_error(q.n, n_items, q.hist_ptr, q.hist_items) : "";
  if (e.empty()) e = own_error(n_items);
  if (e.empty() && !q.fold_in && (q.n < 0 || (q.n > 0 && !q.users))) e = "bad arguments";
  if (!e.empty()) return model_fail(FRECSYS_ERR_INVALID, w + e);
  if (!q.fold_in) {
    r->ids = q.users;
    return FRECSYS_OK;
  }
  if (q.n == 0) return kNoRows;
  frecsys::Csr csr;
  csr.ptr.assign(q.hist_ptr, q.hist_ptr + q.n + 1);
  csr.col.assign(q.hist_items, q.hist_items + q.hist_ptr[q.n]);
  if (projection == kFoldIn) {
    r->dm->FoldIn(csr);
  } else {
    r->dev().LoadEval(csr);
  }
  r->side = FRECSYS_SIDE_EVAL;
  return FRECSYS_OK;
}

// ---- the query entry points, one body per trained / fold-in pair ----

// The trained form leaves k, the outputs and the candidate CSR to the context,
// in whose words they are reported; the fold-in form checks them here, before
// the projection.
int recommend(frecsys_model* m, const std::string& w, const Query& q, int32_t k,
              int32_t exclude_seen, const uint8_t* item_mask, int32_t* items, float* scores) {
  Rows r;
  const auto own = [&](int64_t) { return q.fold_in ? k_items_error(k, q.n, items) : ""; };
  if (int rc = open_query(m, w, q, exclude_seen, own, &r)) return answered(rc);
  return context_status(r.dev(), r.dev().TryRecommend(r.side, r.ids, q.n, k,
                                                      exclude_flag(exclude_seen), item_mask,
                                                      items, scores));
}

// As recommend: the fold-in form checks k, the pool (0: the default) and the
// outputs before the projection, the trained form leaves them to the context.
int recommend_two_stage(frecsys_model* m, const std::string& w, const Query& q, int32_t k,
                        int32_t pool, int32_t exact, int32_t exclude_seen,
                        const uint8_t* item_mask, int32_t* items, float* scores,
                        uint8_t* certified) {
  Rows r;
  const auto own = [&](int64_t) -> std::string {
    if (!q.fold_in) return "";
    const std::string e = k_items_error(k, q.n, items);
    if (!e.empty()) return e;
    return pool != 0 && (pool < k || pool > 1024) ? "pool must be 0 or in [k, 1024]" : "";
  };
  if (int rc = open_query(m, w, q, exclude_seen, own, &r)) return answered(rc);
  return context_status(
      r.dev(), r.dm->RecommendTwoStage(r.side, r.ids, q.n, k, pool,
                                       exclude_flag(exclude_seen) | (exact ? FRECSYS_TS_EXACT : 0),
                                       item_mask, items, scores, certified));
}

int rank_candidates(frecsys_model* m, const std::string& w, const Query& q,
                    const int64_t* cand_ptr, const int32_t* cand_items, int32_t k,
                    int32_t exclude_seen, const uint8_t* item_mask, int32_t* items,
                    float* scores) {
  Rows r;
  const auto own = [&](int64_t n_items) -> std::string {
    if (!q.fold_in) return "";
    if (!cand_ptr || cand_ptr[0] != 0) return "bad arguments";
    const std::string e = k_items_error(k, q.n, items);
    return e.empty() ? cand_args_error(q.n, n_items, cand_ptr, cand_items) : e;
  };
  if (int rc = open_query(m, w, q, exclude_seen, own, &r)) return answered(rc);
  return context_status(
      r.dev(), r.dev().TryRankCandidates(r.side, r.ids, q.n, cand_ptr, cand_items, k,
                                         exclude_flag(exclude_seen), item_mask, items, scores));
}

int recommend_diverse(frecsys_model* m, const std::string& w, const Query& q, int32_t k,
                      int32_t pool, float lam, int32_t raw_scores, int32_t exclude_seen,
                      const uint8_t* item_mask, int32_t* items, float* scores, float* mmr) {
  Rows r;
  const auto own = [&](int64_t) {
    return diverse_args_error(k, pool, lam, raw_scores, q.n, items, scores);
  };
  if (int rc = open_query(m, w, q, exclude_seen, own, &r)) return answered(rc);
  return context_status(r.dev(), r.dm->RecommendDiverse(r.side, r.ids, q.n, k, pool, lam,
                                                        diverse_flags(exclude_seen, raw_scores),
                                                        item_mask, items, scores, mmr));
}

int recommend_dpp(frecsys_model* m, const std::string& w, const Query& q, int32_t k, int32_t pool,
                  float theta, float eps, int32_t raw_scores, int32_t exclude_seen,
                  const uint8_t* item_mask, int32_t* items, float* scores, float* gain) {
  Rows r;
  const auto own = [&](int64_t) {
    return dpp_args_error(k, pool, theta, eps, raw_scores, q.n, items, scores);
  };
  if (int rc = open_query(m, w, q, exclude_seen, own, &r)) return answered(rc);
  return context_status(r.dev(), r.dm->RecommendDpp(r.side, r.ids, q.n, k, pool, theta, eps,
                                                    diverse_flags(exclude_seen, raw_scores),
                                                    item_mask, items, scores, gain));
}

// DeviceModel::Explain / ExplainFoldIn on the opened rows: trained users are
// explained over the training CSR (loaded here if Train() has not: also by a
// call without rows), histories over the EVAL CSR open_query loaded.
int explain(frecsys_model* m, const std::string& w, const Query& q, const int64_t* tgt_ptr,
            const int32_t* tgt_items, int32_t top, float* score, int32_t* top_items,
            float* top_contrib, float* full) {
  Rows r;
  const auto own = [&](int64_t) {
    return (q.fold_in || q.n > 0) && !tgt_ptr ? "bad arguments" : "";
  };
  if (int rc = open_query(m, w, q, /*reads_training=*/1, own, &r, kLoadOnly)) return answered(rc);
  if (!q.fold_in) r.dev().LoadTraining(*m->train);
  r.dev().Gramian(DeviceContext::ITEM);
  const frecsys_solve_params p = r.dm->ExplainParams();
  return context_status(r.dev(), frecsys_explain(r.dev().raw(), r.side, &p, r.ids, q.n, tgt_ptr,
                                                 tgt_items, top, score, top_items, top_contrib,
                                                 full));
}

// The summary of per-row metric values [(2 + 2 na) nk]: mean recall, mean
// ndcg, recall CVaR [na][nk], ndcg CVaR [na][nk] -- EvaluationResult's own
// colwise().mean() and cvar().  The same for every evaluation.
int summarize(int64_t n, const int32_t* k_list, int32_t nk, const float* alpha_list, int32_t na,
              const float* recall, const float* ndcg, float* summary) {
  if (!summary) return FRECSYS_OK;
  frecsys::EvaluationResult er{frecsys::VectorXi(nk), frecsys::VectorXf(na),
                               frecsys::MatrixXf(n, nk), frecsys::MatrixXf(n, nk)};
  for (int32_t q = 0; q < nk; ++q) er.k_list[q] = k_list[q];
  for (int32_t j = 0; j < na; ++j) er.alpha_list[j] = alpha_list[j];
  if (n > 0) {
    std::memcpy(er.recall.data(), recall, sizeof(float) * (size_t)(n * nk));
    std::memcpy(er.ndcg.data(), ndcg, sizeof(float) * (size_t)(n * nk));
  }
  const frecsys::VectorXf mr = er.recall.colwise().mean(), mn = er.ndcg.colwise().mean();
  std::vector<float> col((size_t)n);
  for (int32_t q = 0; q < nk; ++q) {
    summary[q] = mr[q];
    summary[nk + q] = mn[q];
    for (int64_t i = 0; i < n; ++i) col[(size_t)i] = er.recall(i, q);
    const frecsys::VectorXf rc_q = er.cvar(col);
    for (int64_t i = 0; i < n; ++i) col[(size_t)i] = er.ndcg(i, q);
    const frecsys::VectorXf nc_q = er.cvar(col);
    for (int32_t j = 0; j < na; ++j) {
      summary[(size_t)(2 + j) * nk + q] = rc_q[j];
      summary[(size_t)(2 + na + j) * nk + q] = nc_q[j];
    }
  }
  return FRECSYS_OK;
}
int summarize(int64_t n, const Metrics& mt) {
  return summarize(n, mt.k_list, mt.nk, mt.alpha_list, mt.na, mt.recall, mt.ndcg, mt.summary);
}

int evaluate(frecsys_model* m, const std::string& w, const Query& q, const Metrics& mt,
             int32_t exclude_seen) {
  Rows r;
  const auto own = [&](int64_t n_items) { return metrics_args_error(q.n, n_items, mt); };
  const int rc = open_query(m, w, q, exclude_seen, own, &r);
  if (rc == kNoRows) return summarize(q.n, mt);
  if (rc) return rc;
  if (int e = r.dev().TryRankMetrics(r.side, r.ids, q.n, exclude_flag(exclude_seen), nullptr,
                                     mt.gt_ptr, mt.gt_items, mt.k_list, mt.nk, mt.recall,
                                     mt.ndcg))
    return context_status(r.dev(), e);
  return summarize(q.n, mt);
}

// The list evaluations: caller lists (cand_ptr given) or sampled ones.
struct ListEval {
  const int64_t* cand_ptr;
  const int32_t* cand_items;
  int32_t n_neg;
  uint64_t seed;
};

int evaluate_lists(frecsys_model* m, const std::string& w, const Query& q, const ListEval& le,
                   bool sampled, const Metrics& mt, int32_t exclude_seen,
                   const uint8_t* item_mask) {
  // the two list evaluations name themselves together where they need the
  // tuples: checked here, not by open_query under the name in `w`
  if (m && exclude_seen && !q.fold_in)
    if (int rc = needs_data(m, "frecsys_model_evaluate_candidates / _sampled")) return rc;
  Rows r;
  const auto own = [&](int64_t n_items) -> std::string {
    const std::string e = metrics_args_error(q.n, n_items, mt);
    if (!e.empty()) return e;
    if (!sampled) return cand_args_error(q.n, n_items, le.cand_ptr, le.cand_items);
    if (le.n_neg < 0) return "n_neg must not be negative";
    if (le.n_neg > 0 && q.n > INT64_MAX / le.n_neg) return "n * n_neg overflows";
    return "";
  };
  const int rc = open_query(m, w, q, /*reads_training=*/0, own, &r);
  if (rc == kNoRows || (rc == FRECSYS_OK && q.n == 0)) return summarize(q.n, mt);
  if (rc) return rc;
  const int flags = exclude_flag(exclude_seen);
  const int e =
      sampled ? r.dev().TrySampledMetrics(r.side, r.ids, q.n, flags, item_mask, mt.gt_ptr,
                                          mt.gt_items, le.n_neg, le.seed, mt.k_list, mt.nk,
                                          mt.recall, mt.ndcg)
              : r.dev().TryRankCandidatesMetrics(r.side, r.ids, q.n, le.cand_ptr, le.cand_items,
                                                 flags, item_mask, mt.gt_ptr, mt.gt_items,
                                                 mt.k_list, mt.nk, mt.recall, mt.ndcg);
  if (e) return context_status(r.dev(), e);
  return summarize(q.n, mt);
}

// The summary is summarize()'s with one column: mrr in recall's place, auc in
// ndcg's.
int evaluate_ranks(frecsys_model* m, const std::string& w, const Query& q, const int64_t* gt_ptr,
                   const int32_t* gt_items, const float* alpha_list, int32_t na,
                   int32_t exclude_seen, const uint8_t* item_mask, int32_t* rank,
                   int32_t* eligible, float* mrr, float* auc, float* summary) {
  const int32_t one = 1;  // summarize()'s one column
  Rows r;
  const auto own = [&](int64_t n_items) -> std::string {
    std::string e = truth_head_error(q.n, gt_ptr);
    if (e.empty()) e = alpha_error(alpha_list, na);
    if (!e.empty()) return e;
    if (q.n > 0 && !gt_items) return "null gt_items";
    if (q.n > 0 && !rank && !eligible && !mrr && !auc) return "null outputs";
    if (summary && q.n > 0 && (!mrr || !auc)) return "summary needs mrr and auc";
    return truth_rows_error(q.n, n_items, gt_ptr, gt_items);
  };
  const int rc = open_query(m, w, q, exclude_seen, own, &r);
  if (rc == kNoRows || (rc == FRECSYS_OK && q.n == 0))
    return summarize(q.n, &one, 1, alpha_list, na, mrr, auc, summary);
  if (rc) return rc;
  if (int e = r.dev().TryRankPositions(r.side, r.ids, q.n, exclude_flag(exclude_seen), item_mask,
                                       gt_ptr, gt_items, rank, eligible, mrr, auc))
    return context_status(r.dev(), e);
  return summarize(q.n, &one, 1, alpha_list, na, mrr, auc, summary);
}

// The arguments and outputs of a list-quality evaluation (frecsys_hip.h).
struct Quality {
  const int32_t* k_list;
  int32_t nk;
  const float* item_weight;
  const uint8_t* item_mask;
  float* ild;
  float* novelty;
  int64_t* exposure;
  double* summary;
};

// The cases the quality calls reject, before any projection, in this layer's
// words; max_k: the longest list a cut-off may ask for.  The same checks in the
// same order as quality_args_error of csrc/serve.hip (32 and 1024 are its
// kMetricMaxCutoffs and kMetricMaxK, frecsys_hip.h's limits): keep the two in
// step.  The context runs them again, as it does for every call.
std::string quality_args_error(const Quality& ql, int32_t max_k, int64_t n_items, bool others) {
  if (!ql.k_list || ql.nk < 1 || ql.nk > 32) return "k_list must hold 1 to 32 cut-offs";
  for (int32_t q = 0; q < ql.nk; ++q)
    if (ql.k_list[q] < 1 || ql.k_list[q] > max_k)
      return "cut-offs must be in [1, " + std::to_string(max_k) + "]";
  if (!ql.ild && !ql.novelty && !ql.exposure && !others) return "null outputs";
  if (ql.novelty && !ql.item_weight) return "novelty needs item_weight";
  if (ql.item_weight && !ql.novelty) return "item_weight without a novelty output";
  if (ql.item_weight)
    for (int64_t j = 0; j < n_items; ++j)
      if (!std::isfinite(ql.item_weight[j]))
        return "item_weight[" + std::to_string(j) + "] is not finite";
  return "";
}

// summary[0 .. 4 nk): the mean ILD and the mean novelty per cut-off (double sums
// of the per-row values in row order, over n), then coverage and Gini of each
// exposure row among the masked items (frecsys_exposure_summary); 0 where the
// output was not asked for.
int summarize_quality(int64_t n, int64_t n_items, const Quality& ql) {
  if (!ql.summary) return FRECSYS_OK;
  const int32_t nk = ql.nk;
  std::fill(ql.summary, ql.summary + 4 * (size_t)nk, 0.0);
  for (int32_t q = 0; q < nk; ++q) {
    double si = 0.0, sn = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      if (ql.ild) si += (double)ql.ild[i * nk + q];
      if (ql.novelty) sn += (double)ql.novelty[i * nk + q];
    }
    if (n > 0) {
      ql.summary[q] = si / (double)n;
      ql.summary[nk + q] = sn / (double)n;
    }
    if (ql.exposure)
      if (int rc = frecsys_exposure_summary(ql.exposure + (int64_t)q * n_items, n_items,
                                            ql.item_mask, &ql.summary[2 * nk + q],
                                            &ql.summary[3 * nk + q], nullptr, nullptr))
        return model_fail(rc, frecsys_last_error(nullptr));
  }
  return FRECSYS_OK;
}

// The Recall / NDCG part of a quality evaluation: absent (gt_ptr null, recall
// and ndcg null) or whole.
struct Truth {
  const int64_t* gt_ptr;
  const int32_t* gt_items;
  const float* alpha_list;
  int32_t na;
  float* recall;
  float* ndcg;
};

// summary[4 nk .. (6 + 2 na) nk): summarize()'s floats, widened; 0 without a
// ground truth.
void summarize_truth(int64_t n, const Quality& ql, const Truth& tr) {
  if (!ql.summary) return;
  const size_t len = (size_t)(2 + 2 * tr.na) * ql.nk;
  std::vector<float> tmp(len, 0.0f);
  if (tr.gt_ptr)
    summarize(n, ql.k_list, ql.nk, tr.alpha_list, tr.na, tr.recall, tr.ndcg, tmp.data());
  for (size_t t = 0; t < len; ++t) ql.summary[4 * (size_t)ql.nk + t] = (double)tmp[t];
}

int evaluate_quality(frecsys_model* m, const std::string& w, const Query& q, const Quality& ql,
                     int32_t pool, float lam, int32_t raw_scores, const Truth& tr,
                     int32_t exclude_seen) {
  Rows r;
  int64_t items = 0;
  const auto own = [&](int64_t n_items) -> std::string {
    items = n_items;
    std::string e = quality_args_error(ql, 1024, n_items, tr.recall || tr.ndcg);
    if (!e.empty()) return e;
    if (pool < 0 || pool > 1024) return "pool must be 0 or in [1, 1024]";
    if (raw_scores != 0 && raw_scores != 1) return "raw_scores must be 0 or 1";
    if (pool > 0) {
      for (int32_t c = 0; c < ql.nk; ++c)
        if (ql.k_list[c] > pool) return "cut-offs must not exceed pool";
      if (!(lam >= 0.0f && lam <= 1.0f)) return "lam must be in [0, 1]";
    } else if (raw_scores) {
      return "raw_scores without a pool";
    }
    if (!(e = alpha_error(tr.alpha_list, tr.na)).empty()) return e;
    if (!tr.gt_ptr) return tr.recall || tr.ndcg ? "recall / ndcg need a ground truth" : "";
    if (!tr.recall || !tr.ndcg) return "a ground truth needs recall and ndcg";
    if (!(e = truth_head_error(q.n, tr.gt_ptr)).empty()) return e;
    if (q.n > 0 && !tr.gt_items) return "null gt_items";
    return truth_rows_error(q.n, n_items, tr.gt_ptr, tr.gt_items);
  };
  const int rc = open_query(m, w, q, exclude_seen, own, &r);
  if (rc && rc != kNoRows) return rc;
  if (rc == kNoRows) {
    if (ql.exposure) std::fill(ql.exposure, ql.exposure + (int64_t)ql.nk * items, (int64_t)0);
  } else if (int e = frecsys_rank_quality(
                 r.dev().raw(), r.side, r.ids, q.n, exclude_flag(exclude_seen), ql.item_mask,
                 ql.k_list, ql.nk, pool, lam, raw_scores ? FRECSYS_DIV_RAW_SCORES : 0,
                 ql.item_weight, tr.gt_ptr, tr.gt_items, ql.ild, ql.novelty, tr.recall, tr.ndcg,
                 ql.exposure)) {
    return context_status(r.dev(), e);
  }
  if (int e = summarize_quality(q.n, items, ql)) return e;
  summarize_truth(q.n, ql, tr);
  return FRECSYS_OK;
}

int model_similar(frecsys_model* m, const char* what, int side, const int64_t* rows, int64_t n,
                  int32_t k, int32_t flags, const uint8_t* mask, int32_t* ids, float* scores) {
  if (!m || n < 0 || (n > 0 && !ids))
    return model_fail(FRECSYS_ERR_INVALID, std::string(what) + ": bad arguments");
  DeviceContext& dev = frecsys::AsDeviceModel(m->rec.get())->device();
  return context_status(dev, dev.TrySimilar(side, rows, n, k, flags, mask, ids, scores));
}

}  // namespace

extern "C" {

int frecsys_model_recommend(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                            int32_t exclude_seen, const uint8_t* item_mask, int32_t* items,
                            float* scores) {
  return recommend(m, "frecsys_model_recommend: ", trained(users, n), k, exclude_seen, item_mask,
                   items, scores);
}

int frecsys_model_recommend_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                    const int32_t* hist_items, int64_t n, int32_t k,
                                    int32_t exclude_seen, const uint8_t* item_mask,
                                    int32_t* items, float* scores) {
  return recommend(m, "frecsys_model_recommend_fold_in: ", unseen(hist_ptr, hist_items, n), k,
                   exclude_seen, item_mask, items, scores);
}

int frecsys_model_recommend_two_stage(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                                      int32_t pool, int32_t exact, int32_t exclude_seen,
                                      const uint8_t* item_mask, int32_t* items, float* scores,
                                      uint8_t* certified) {
  return recommend_two_stage(m, "frecsys_model_recommend_two_stage: ", trained(users, n), k, pool,
                             exact, exclude_seen, item_mask, items, scores, certified);
}

int frecsys_model_recommend_two_stage_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                              const int32_t* hist_items, int64_t n, int32_t k,
                                              int32_t pool, int32_t exact, int32_t exclude_seen,
                                              const uint8_t* item_mask, int32_t* items,
                                              float* scores, uint8_t* certified) {
  return recommend_two_stage(m, "frecsys_model_recommend_two_stage_fold_in: ",
                             unseen(hist_ptr, hist_items, n), k, pool, exact, exclude_seen,
                             item_mask, items, scores, certified);
}

int frecsys_model_score(frecsys_model* m, const int64_t* users, const int32_t* items, int64_t n,
                        float* scores) {
  if (!m || n < 0 || (n > 0 && (!users || !items || !scores)))
    return model_fail(FRECSYS_ERR_INVALID, "frecsys_model_score: bad arguments");
  DeviceContext& dev = frecsys::AsDeviceModel(m->rec.get())->device();
  return context_status(dev, dev.TryScorePairs(FRECSYS_SIDE_USER, users, items, n, scores));
}

int frecsys_model_explain(frecsys_model* m, const int64_t* users, int64_t n,
                          const int64_t* tgt_ptr, const int32_t* tgt_items, int32_t top,
                          float* score, int32_t* top_items, float* top_contrib, float* full) {
  return explain(m, "frecsys_model_explain: ", trained(users, n), tgt_ptr, tgt_items, top, score,
                 top_items, top_contrib, full);
}

int frecsys_model_explain_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                  const int32_t* hist_items, int64_t n, const int64_t* tgt_ptr,
                                  const int32_t* tgt_items, int32_t top, float* score,
                                  int32_t* top_items, float* top_contrib, float* full) {
  return explain(m, "frecsys_model_explain_fold_in: ", unseen(hist_ptr, hist_items, n), tgt_ptr,
                 tgt_items, top, score, top_items, top_contrib, full);
}

int frecsys_model_rank_candidates(frecsys_model* m, const int64_t* users, int64_t n,
                                  const int64_t* cand_ptr, const int32_t* cand_items, int32_t k,
                                  int32_t exclude_seen, const uint8_t* item_mask, int32_t* items,
                                  float* scores) {
  return rank_candidates(m, "frecsys_model_rank_candidates: ", trained(users, n), cand_ptr,
                         cand_items, k, exclude_seen, item_mask, items, scores);
}

int frecsys_model_rank_candidates_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                          const int32_t* hist_items, int64_t n,
                                          const int64_t* cand_ptr, const int32_t* cand_items,
                                          int32_t k, int32_t exclude_seen,
                                          const uint8_t* item_mask, int32_t* items,
                                          float* scores) {
  return rank_candidates(m, "frecsys_model_rank_candidates_fold_in: ",
                         unseen(hist_ptr, hist_items, n), cand_ptr, cand_items, k, exclude_seen,
                         item_mask, items, scores);
}

int frecsys_model_similar_items(frecsys_model* m, const int64_t* items, int64_t n, int32_t k,
                                int32_t flags, const uint8_t* item_mask, int32_t* ids,
                                float* scores) {
  return model_similar(m, "frecsys_model_similar_items", FRECSYS_SIDE_ITEM, items, n, k, flags,
                       item_mask, ids, scores);
}

int frecsys_model_similar_users(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                                int32_t flags, const uint8_t* user_mask, int32_t* ids,
                                float* scores) {
  return model_similar(m, "frecsys_model_similar_users", FRECSYS_SIDE_USER, users, n, k, flags,
                       user_mask, ids, scores);
}

int frecsys_model_audience(frecsys_model* m, const int64_t* items, int64_t n, int32_t k,
                           int32_t exclude_seen, const uint8_t* user_mask, int32_t* users,
                           float* scores) {
  const std::string w = "frecsys_model_audience: ";
  if (!m || n < 0 || (n > 0 && !users)) return model_fail(FRECSYS_ERR_INVALID, w + "bad arguments");
  if (exclude_seen)
    if (int rc = needs_data(m, "frecsys_model_audience")) return rc;
  DeviceContext& dev = frecsys::AsDeviceModel(m->rec.get())->device();
  if (exclude_seen && n > 0) {
    // the ITEM-side CSR, if no Train() has loaded it yet -- behind the checks
    // of k and the item ids, so that a rejected call makes no device call
    const int64_t n_items = dev.rows(DeviceContext::ITEM);
    if (k < 1 || k > 1024) return model_fail(FRECSYS_ERR_INVALID, w + "k must be in [1, 1024]");
    if (!items && n > n_items)
      return model_fail(FRECSYS_ERR_INVALID, w + "more rows than the side has");
    for (int64_t i = 0; items && i < n; ++i)
      if (items[i] < 0 || items[i] >= n_items)
        return model_fail(FRECSYS_ERR_INVALID,
                          w + "row id " + std::to_string(items[i]) + " out of range");
    dev.LoadTraining(*m->train);
  }
  return context_status(dev, dev.TryAudience(items, n, k,
                                             exclude_seen ? FRECSYS_AUD_EXCLUDE_HISTORY : 0,
                                             user_mask, users, scores));
}

int frecsys_model_evaluate(frecsys_model* m, const int64_t* users, int64_t n,
                           const int64_t* gt_ptr, const int32_t* gt_items, const int32_t* k_list,
                           int32_t nk, const float* alpha_list, int32_t na, int32_t exclude_seen,
                           float* recall, float* ndcg, float* summary) {
  return evaluate(m, "frecsys_model_evaluate: ", trained(users, n),
                  Metrics{gt_ptr, gt_items, k_list, nk, alpha_list, na, recall, ndcg, summary},
                  exclude_seen);
}

int frecsys_model_evaluate_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                   const int32_t* hist_items, int64_t n, const int64_t* gt_ptr,
                                   const int32_t* gt_items, const int32_t* k_list, int32_t nk,
                                   const float* alpha_list, int32_t na, int32_t exclude_seen,
                                   float* recall, float* ndcg, float* summary) {
  return evaluate(m, "frecsys_model_evaluate_fold_in: ", unseen(hist_ptr, hist_items, n),
                  Metrics{gt_ptr, gt_items, k_list, nk, alpha_list, na, recall, ndcg, summary},
                  exclude_seen);
}

int frecsys_model_evaluate_ranks(frecsys_model* m, const int64_t* users, int64_t n,
                                 const int64_t* gt_ptr, const int32_t* gt_items,
                                 const float* alpha_list, int32_t na, int32_t exclude_seen,
                                 const uint8_t* item_mask, int32_t* rank, int32_t* eligible,
                                 float* mrr, float* auc, float* summary) {
  return evaluate_ranks(m, "frecsys_model_evaluate_ranks: ", trained(users, n), gt_ptr, gt_items,
                        alpha_list, na, exclude_seen, item_mask, rank, eligible, mrr, auc,
                        summary);
}

int frecsys_model_evaluate_ranks_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                         const int32_t* hist_items, int64_t n,
                                         const int64_t* gt_ptr, const int32_t* gt_items,
                                         const float* alpha_list, int32_t na,
                                         int32_t exclude_seen, const uint8_t* item_mask,
                                         int32_t* rank, int32_t* eligible, float* mrr,
                                         float* auc, float* summary) {
  return evaluate_ranks(m, "frecsys_model_evaluate_ranks_fold_in: ",
                        unseen(hist_ptr, hist_items, n), gt_ptr, gt_items, alpha_list, na,
                        exclude_seen, item_mask, rank, eligible, mrr, auc, summary);
}

int frecsys_model_evaluate_candidates(frecsys_model* m, const int64_t* users, int64_t n,
                                      const int64_t* cand_ptr, const int32_t* cand_items,
                                      const int64_t* gt_ptr, const int32_t* gt_items,
                                      const int32_t* k_list, int32_t nk, const float* alpha_list,
                                      int32_t na, int32_t exclude_seen, const uint8_t* item_mask,
                                      float* recall, float* ndcg, float* summary) {
  return evaluate_lists(m, "frecsys_model_evaluate_candidates: ", trained(users, n),
                        ListEval{cand_ptr, cand_items, 0, 0}, false,
                        Metrics{gt_ptr, gt_items, k_list, nk, alpha_list, na, recall, ndcg,
                                summary},
                        exclude_seen, item_mask);
}

int frecsys_model_evaluate_candidates_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                              const int32_t* hist_items, int64_t n,
                                              const int64_t* cand_ptr, const int32_t* cand_items,
                                              const int64_t* gt_ptr, const int32_t* gt_items,
                                              const int32_t* k_list, int32_t nk,
                                              const float* alpha_list, int32_t na,
                                              int32_t exclude_seen, const uint8_t* item_mask,
                                              float* recall, float* ndcg, float* summary) {
  return evaluate_lists(m, "frecsys_model_evaluate_candidates_fold_in: ",
                        unseen(hist_ptr, hist_items, n), ListEval{cand_ptr, cand_items, 0, 0},
                        false,
                        Metrics{gt_ptr, gt_items, k_list, nk, alpha_list, na, recall, ndcg,
                                summary},
                        exclude_seen, item_mask);
}

int frecsys_model_evaluate_sampled(frecsys_model* m, const int64_t* users, int64_t n,
                                   const int64_t* gt_ptr, const int32_t* gt_items, int32_t n_neg,
                                   uint64_t seed, const int32_t* k_list, int32_t nk,
                                   const float* alpha_list, int32_t na, int32_t exclude_seen,
                                   const uint8_t* item_mask, float* recall, float* ndcg,
                                   float* summary) {
  return evaluate_lists(m, "frecsys_model_evaluate_sampled: ", trained(users, n),
                        ListEval{nullptr, nullptr, n_neg, seed}, true,
                        Metrics{gt_ptr, gt_items, k_list, nk, alpha_list, na, recall, ndcg,
                                summary},
                        exclude_seen, item_mask);
}

int frecsys_model_evaluate_sampled_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                           const int32_t* hist_items, int64_t n,
                                           const int64_t* gt_ptr, const int32_t* gt_items,
                                           int32_t n_neg, uint64_t seed, const int32_t* k_list,
                                           int32_t nk, const float* alpha_list, int32_t na,
                                           int32_t exclude_seen, const uint8_t* item_mask,
                                           float* recall, float* ndcg, float* summary) {
  return evaluate_lists(m, "frecsys_model_evaluate_sampled_fold_in: ",
                        unseen(hist_ptr, hist_items, n), ListEval{nullptr, nullptr, n_neg, seed},
                        true,
                        Metrics{gt_ptr, gt_items, k_list, nk, alpha_list, na, recall, ndcg,
                                summary},
                        exclude_seen, item_mask);
}

int frecsys_model_recommend_diverse(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                                    int32_t pool, float lam, int32_t raw_scores,
                                    int32_t exclude_seen, const uint8_t* item_mask,
                                    int32_t* items, float* scores, float* mmr) {
  return recommend_diverse(m, "frecsys_model_recommend_diverse: ", trained(users, n), k, pool, lam,
                           raw_scores, exclude_seen, item_mask, items, scores, mmr);
}

int frecsys_model_recommend_diverse_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                            const int32_t* hist_items, int64_t n, int32_t k,
                                            int32_t pool, float lam, int32_t raw_scores,
                                            int32_t exclude_seen, const uint8_t* item_mask,
                                            int32_t* items, float* scores, float* mmr) {
  return recommend_diverse(m, "frecsys_model_recommend_diverse_fold_in: ",
                           unseen(hist_ptr, hist_items, n), k, pool, lam, raw_scores, exclude_seen,
                           item_mask, items, scores, mmr);
}

int frecsys_model_diversify(frecsys_model* m, const int32_t* lists, const float* list_scores,
                            int64_t n, int32_t pool, int32_t k, float lam, int32_t raw_scores,
                            int32_t* items, float* scores, float* mmr) {
  const std::string w = "frecsys_model_diversify: ";
  if (!m || n < 0 || (n > 0 && (!lists || !list_scores)))
    return model_fail(FRECSYS_ERR_INVALID, w + "bad arguments");
  const std::string e = diverse_args_error(k, pool, lam, raw_scores, n, items, scores);
  if (!e.empty()) return model_fail(FRECSYS_ERR_INVALID, w + e);
  frecsys::detail::DeviceModel* dm = frecsys::AsDeviceModel(m->rec.get());
  return context_status(dm->device(), dm->Diversify(lists, list_scores, n, pool, k, lam,
                                                    diverse_flags(0, raw_scores), items, scores,
                                                    mmr));
}

int frecsys_model_recommend_dpp(frecsys_model* m, const int64_t* users, int64_t n, int32_t k,
                                int32_t pool, float theta, float eps, int32_t raw_scores,
                                int32_t exclude_seen, const uint8_t* item_mask, int32_t* items,
                                float* scores, float* gain) {
  return recommend_dpp(m, "frecsys_model_recommend_dpp: ", trained(users, n), k, pool, theta, eps,
                       raw_scores, exclude_seen, item_mask, items, scores, gain);
}

int frecsys_model_recommend_dpp_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                        const int32_t* hist_items, int64_t n, int32_t k,
                                        int32_t pool, float theta, float eps, int32_t raw_scores,
                                        int32_t exclude_seen, const uint8_t* item_mask,
                                        int32_t* items, float* scores, float* gain) {
  return recommend_dpp(m, "frecsys_model_recommend_dpp_fold_in: ", unseen(hist_ptr, hist_items, n),
                       k, pool, theta, eps, raw_scores, exclude_seen, item_mask, items, scores,
                       gain);
}

int frecsys_model_diversify_dpp(frecsys_model* m, const int32_t* lists, const float* list_scores,
                                int64_t n, int32_t pool, int32_t k, float theta, float eps,
                                int32_t raw_scores, int32_t* items, float* scores, float* gain) {
  const std::string w = "frecsys_model_diversify_dpp: ";
  if (!m || n < 0 || (n > 0 && (!lists || !list_scores)))
    return model_fail(FRECSYS_ERR_INVALID, w + "bad arguments");
  const std::string e = dpp_args_error(k, pool, theta, eps, raw_scores, n, items, scores);
  if (!e.empty()) return model_fail(FRECSYS_ERR_INVALID, w + e);
  frecsys::detail::DeviceModel* dm = frecsys::AsDeviceModel(m->rec.get());
  return context_status(dm->device(), dm->DiversifyDpp(lists, list_scores, n, pool, k, theta, eps,
                                                       diverse_flags(0, raw_scores), items, scores,
                                                       gain));
}

int frecsys_model_evaluate_quality(frecsys_model* m, const int64_t* users, int64_t n,
                                   const int32_t* k_list, int32_t nk, int32_t pool, float lam,
                                   int32_t raw_scores, const float* item_weight,
                                   const int64_t* gt_ptr, const int32_t* gt_items,
                                   const float* alpha_list, int32_t na, int32_t exclude_seen,
                                   const uint8_t* item_mask, float* ild, float* novelty,
                                   float* recall, float* ndcg, int64_t* exposure,
                                   double* summary) {
  return evaluate_quality(m, "frecsys_model_evaluate_quality: ", trained(users, n),
                          Quality{k_list, nk, item_weight, item_mask, ild, novelty, exposure,
                                  summary},
                          pool, lam, raw_scores,
                          Truth{gt_ptr, gt_items, alpha_list, na, recall, ndcg}, exclude_seen);
}

int frecsys_model_evaluate_quality_fold_in(frecsys_model* m, const int64_t* hist_ptr,
                                           const int32_t* hist_items, int64_t n,
                                           const int32_t* k_list, int32_t nk, int32_t pool,
                                           float lam, int32_t raw_scores,
                                           const float* item_weight, const int64_t* gt_ptr,
                                           const int32_t* gt_items, const float* alpha_list,
                                           int32_t na, int32_t exclude_seen,
                                           const uint8_t* item_mask, float* ild, float* novelty,
                                           float* recall, float* ndcg, int64_t* exposure,
                                           double* summary) {
  return evaluate_quality(m, "frecsys_model_evaluate_quality_fold_in: ",
                          unseen(hist_ptr, hist_items, n),
                          Quality{k_list, nk, item_weight, item_mask, ild, novelty, exposure,
                                  summary},
                          pool, lam, raw_scores,
                          Truth{gt_ptr, gt_items, alpha_list, na, recall, ndcg}, exclude_seen);
}

int frecsys_model_list_quality(frecsys_model* m, const int32_t* lists, int64_t n, int32_t list_k,
                               const int32_t* k_list, int32_t nk, const float* item_weight,
                               const uint8_t* item_mask, float* ild, float* novelty,
                               int64_t* exposure, double* summary) {
  const std::string w = "frecsys_model_list_quality: ";
  if (!m || n < 0 || list_k < 1 || (n > 0 && !lists))
    return model_fail(FRECSYS_ERR_INVALID, w + "bad arguments");
  DeviceContext& dev = frecsys::AsDeviceModel(m->rec.get())->device();
  const int64_t n_items = dev.rows(DeviceContext::ITEM);
  const Quality ql{k_list, nk, item_weight, item_mask, ild, novelty, exposure, summary};
  const std::string e = quality_args_error(ql, std::min<int32_t>(1024, list_k), n_items, false);
  if (!e.empty()) return model_fail(FRECSYS_ERR_INVALID, w + e);
  if (int rc = frecsys_lists_quality(dev.raw(), lists, n, list_k, k_list, nk, item_weight, ild,
                                     novelty, exposure))
    return context_status(dev, rc);
  return summarize_quality(n, n_items, ql);
}

void frecsys_model_destroy(frecsys_model* m) { delete m; }

const char* frecsys_model_last_error(void) { return g_model_error.c_str(); }

}  // extern "C"
