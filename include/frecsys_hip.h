/*
 * frecsys_hip.h -- C-ABI of libfrecsys_hip.so, the MI355X (gfx950) solve
 * loop behind iALS / ERM-MF / CVaR-MF / SAFER2.
 *
 * Plain C types only (no torch / HIP / RCCL types).  Every call is
 * synchronous on return (the reference's Step* functions block until all
 * threads join, ials.h:359-361) and returns FRECSYS_OK (0) or an error code;
 * frecsys_last_error() gives the message.  The library owns every device
 * buffer (embeddings, Gramians, CSR, workspaces); they stay resident in HBM
 * across epochs.  Host pointers passed in are never retained after a call.
 *
 * Which reference interface each entry point replaces (reference paths are
 * relative to riktor/safer2-recommender):
 *
 *   frecsys_ctx_create / destroy  -- the model ctor's allocation of
 *       user_embedding_ / item_embedding_ / item_gramian_
 *       (ials.h:39-45, safer2.h:37-48, erm_mf.h:36-44, cvar_mf.h:36-43)
 *   frecsys_load_csr              -- Dataset::by_user()/by_item()
 *       (dataset.h:27-32, 83-92): the per-entity SpVector histories, as CSR
 *       rows kept in file order
 *   frecsys_set/get_embeddings    -- init_matrix writes (recommender.h:61-67)
 *       and item_embedding() reads (ials.h:410-412)
 *   frecsys_init_embeddings       -- std::mt19937 + normal_distribution<float>
 *       init of U then V (ials.h:47-51, recommender.h:61-67), seeded
 *   frecsys_gramian               -- `X.transpose() * X` (ials.h:321,
 *       ials.h:371, safer2.h:55, safer2.h:294-295) and the weighted
 *       `U^T (U .* omega)` (safer2.h:504-509, erm_mf.h:462-467,
 *       cvar_mf.h:484-489)
 *   frecsys_solve_side            -- Step / StepU / StepV / StepU_eval with
 *       their static per-entity Project / ProjectU / ProjectV /
 *       ProjectU_eval (ials.h:88-144 + 317-365; safer2.h:104-221 + 437-555;
 *       erm_mf.h:91-210 + 397-513; cvar_mf.h:88-229 + 427-538 + 645-692)
 *   frecsys_solve_side_cg         -- the same drivers with use_cg: the
 *       Eigen::ConjugateGradient branch of Project / ProjectU / ProjectV
 *       (ials.h:133-139; safer2.h:152-157, 210-215)
 *   frecsys_user_loss             -- ComputeUserLoss / ComputeLoss
 *       (ials.h:70-86 + 367-408; safer2.h:85-101 + 558-596)
 *   frecsys_comm_* / frecsys_partition -- new: the reference has no
 *       multi-device path; these shard the entity loop of the Step* drivers
 *       (safer2.h:447-487) across one process per GPU (RCCL over xGMI).
 */
#ifndef FRECSYS_HIP_H_
#define FRECSYS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define FRECSYS_OK 0
#define FRECSYS_ERR_INVALID 1     /* bad argument / state */
#define FRECSYS_ERR_HIP 2         /* HIP runtime error */
#define FRECSYS_ERR_RCCL 3        /* RCCL error */
#define FRECSYS_ERR_NOT_SPD 4     /* LLT failed (reference: assert, ials.h:141);
                                     entity id via frecsys_last_error_entity */
#define FRECSYS_ERR_NAN 5         /* NaN detected (reference: LOG(ERROR) + exit) */
#define FRECSYS_ERR_UNSUPPORTED 6 /* e.g. dim beyond the kernels built */
#define FRECSYS_ERR_NO_DEVICE 7   /* no HIP device visible */
#define FRECSYS_ERR_IO 8          /* open / read / write / rename of a file failed
                                     (model checkpoints, frecsys_model.h) */

/* ---- sides ---- */
#define FRECSYS_SIDE_USER 0 /* train by_user: rows = users, cols = items */
#define FRECSYS_SIDE_ITEM 1 /* train by_item: rows = items, cols = users */
#define FRECSYS_SIDE_EVAL 2 /* fold-in users (EvaluateDataset, ials.h:148-174);
                               rows = compacted eval users, cols = items */

/* ---- per-entity solve kinds ---- */
#define FRECSYS_KIND_IALS 0        /* ials.h:88-144 */
#define FRECSYS_KIND_WEIGHTED_U 1  /* safer2.h:104-163, erm_mf.h:91-151,
                                      cvar_mf.h:182-229 (ProjectU_eval) */
#define FRECSYS_KIND_WEIGHTED_V 2  /* safer2.h:166-221, erm_mf.h:153-210 */
#define FRECSYS_KIND_CVAR_GRAD_U 3 /* cvar_mf.h:88-134 */
#define FRECSYS_KIND_CVAR_GRAD_V 4 /* cvar_mf.h:136-180 */

typedef struct frecsys_ctx frecsys_ctx;

typedef struct {
  int32_t dim;           /* embedding dimension (reference --dim) */
  int32_t device;        /* HIP device ordinal; -1 = current device */
  int32_t parity_quirks; /* 1: reproduce reference quirks */
  int32_t reserved;
  int64_t n_users;       /* max_user + 1 (run_model.cc:240) */
  int64_t n_items;       /* max_item + 1 */
} frecsys_config;

typedef struct {
  int32_t kind;            /* FRECSYS_KIND_* */
  float reg;               /* l2_reg */
  float reg_exp;           /* l2_reg_exp (iALS only, ials.h:312-314) */
  float unobserved_weight; /* uobs_weight */
  float alpha;             /* alpha (ItemRegularizationValue, safer2.h:430) */
  float stepsize;          /* CVaR-MF eta (cvar_mf.h:133) */
  int32_t from_snapshot;   /* 1: X = snapshot of the other side (CVaR StepV
                              uses the pre-step U, cvar_mf.h:282,294) */
  int32_t lambda_is_reg;   /* 1: use `reg` itself as every entity's lambda
                              (the static Project* API receives the final
                              lambda, ials.h:88-90) */
  const float* entity_weight; /* host [rows of side]: omega_u (WEIGHTED_U,
                                 CVAR_GRAD_U); NULL -> 1 */
  const float* entity_reg;    /* host [rows of side]: item_reg_[v]
                                 (WEIGHTED_V, CVAR_GRAD_V) */
  const float* other_weight;  /* host [rows of other side]: nu_u =
                                 omega_u / |H_u| (WEIGHTED_V, CVAR_GRAD_V) */
} frecsys_solve_params;

/* ---- context ---- */
int frecsys_device_count(int32_t* n);
int frecsys_ctx_create(const frecsys_config* cfg, frecsys_ctx** out);
void frecsys_ctx_destroy(frecsys_ctx* ctx);
/* Message of the last error on ctx (ctx may be NULL: last global error). */
const char* frecsys_last_error(const frecsys_ctx* ctx);
/* Entity (row of the side) of the last FRECSYS_ERR_NOT_SPD, or -1. */
int64_t frecsys_last_error_entity(const frecsys_ctx* ctx);
/* Padded leading dimension used on device (dim rounded up). */
int32_t frecsys_padded_dim(int32_t dim);

/* ---- multi-GPU (one process per GPU) ---- */
/* Host-only: contiguous nnz-balanced split of rows into nparts ranges,
 * bounds[0]=0 .. bounds[nparts]=n_rows (safe to call without a GPU). */
int frecsys_partition(int64_t n_rows, const int64_t* row_ptr, int32_t nparts,
                      int64_t* bounds);
/* Host-only: the partition-independent Gramian plan of n_rows rows at
 * `dim` (frecsys_gramian): rows per leaf, leaves, groups (group g = leaves
 * [g*n_leaves/n_groups, (g+1)*n_leaves/n_groups)) and the groups
 * [own_lo, own_hi) rank `rank` of `world` computes.  Any output may be NULL. */
int frecsys_gram_plan(int32_t dim, int64_t n_rows, int32_t world, int32_t rank,
                      int64_t* rows_per_leaf, int64_t* n_leaves, int32_t* n_groups,
                      int32_t* own_lo, int32_t* own_hi);
/* RCCL unique id (128 bytes) -- call on rank 0, broadcast to the others. */
int frecsys_comm_unique_id(uint8_t id[128]);
/* Join rank `rank` of `world`.  id != NULL: RCCL communicator; the library
 * all-reduces the Gramians and all-gathers factor rows / losses itself.
 * id == NULL (world > 1): external exchange -- no communicator; every call
 * works on this rank's shard only (frecsys_gramian returns the partial Gramian
 * over the rank's rows, solve_side / user_loss write only its rows) and the
 * caller performs the exchange (frecsys_set_gramian, set_embeddings), e.g.
 * over its own MPI / gloo transport or, in tests, several contexts of one
 * process sharing a device. */
int frecsys_comm_init(frecsys_ctx* ctx, int32_t world, int32_t rank,
                      const uint8_t id[128]);
/* World size and rank the context joined, and the rank count of its RCCL
 * communicator (ncclCommCount; 0 without one). */
int frecsys_comm_world(const frecsys_ctx* ctx, int32_t* world, int32_t* rank,
                       int32_t* comm_ranks);
/* Row range [lo, hi) of `side` owned by this rank (after load_csr). */
int frecsys_shard_range(const frecsys_ctx* ctx, int32_t side, int64_t* lo,
                        int64_t* hi);

/* ---- data ---- */
int frecsys_load_csr(frecsys_ctx* ctx, int32_t side, int64_t n_rows,
                     const int64_t* row_ptr, const int32_t* col);
int frecsys_set_embeddings(frecsys_ctx* ctx, int32_t side, const float* host,
                           int64_t ld);
int frecsys_get_embeddings(frecsys_ctx* ctx, int32_t side, float* host,
                           int64_t ld);
/* Seeded init of U then V, identical to std::mt19937{seed} +
 * std::normal_distribution<float>(0, stdev/sqrt(dim)) per matrix. */
int frecsys_init_embeddings(frecsys_ctx* ctx, uint32_t seed, float stdev);
/* Copy the current embeddings of side into its snapshot slot. */
int frecsys_snapshot(frecsys_ctx* ctx, int32_t side);

/* ---- compute ---- */
/* G[side] = X^T diag(w) X over all rows of side's embeddings (or of its
 * snapshot).  Partition-independent: the rows are cut into fixed leaves and
 * the leaves into n_groups fixed groups (frecsys_gram_groups; the cut depends
 * only on the row count); each rank computes the slabs of its own groups,
 * the slabs are all-gathered over RCCL and every rank sums them in group
 * order, so G is bitwise the same at every world size.  Without a
 * communicator at world > 1 (external exchange) G is the sum of this rank's
 * groups only; the caller exchanges the group slabs (frecsys_get_gram_groups
 * / frecsys_set_gram_groups) or partial Gramians (frecsys_set_gramian).
 * weights: host [rows of side] or NULL.  host_out (dim x dim, row-major) may
 * be NULL. */
int frecsys_gramian(frecsys_ctx* ctx, int32_t side, const float* weights,
                    int32_t from_snapshot, float* host_out);
/* Read G[side] as the context holds it (dim x dim, leading dim ld). */
int frecsys_get_gramian(frecsys_ctx* ctx, int32_t side, float* host, int64_t ld);
/* The Gramian plan of `side`: group count, the groups [own_lo, own_hi) this
 * rank computes, floats per group slab (any pointer may be NULL). */
int frecsys_gram_groups(const frecsys_ctx* ctx, int32_t side, int32_t* n_groups,
                        int32_t* own_lo, int32_t* own_hi, int64_t* floats_per_group);
/* All group slabs of the last Gramian of `side` formed here (host
 * [n_groups * floats_per_group]; at world > 1 without a communicator, the
 * other ranks' slabs are zero). */
int frecsys_get_gram_groups(frecsys_ctx* ctx, int32_t side, float* host);
/* G[side] = the group-order sum of the given slabs (every group's slab, as
 * gathered from the owners): the external-exchange completion of
 * frecsys_gramian. */
int frecsys_set_gram_groups(frecsys_ctx* ctx, int32_t side, const float* host);
/* Overwrite G[side] with a host dim x dim matrix (row-major, leading dim
 * ld) -- the static Project* entry points take an arbitrary Gramian. */
int frecsys_set_gramian(frecsys_ctx* ctx, int32_t side, const float* host,
                        int64_t ld);
/* Solve every row of `side` owned by this rank against the other side's
 * embeddings and G[other side]; rows with an empty history are left
 * untouched.  USER/ITEM results are then all-gathered across ranks.  EVAL
 * solves against ITEM and writes the EVAL embeddings. */
int frecsys_solve_side(frecsys_ctx* ctx, int32_t side,
                       const frecsys_solve_params* params);
/* ---- conjugate-gradient solve (--use_cg) ----
 * The `use_cg` branch of the reference's Project / ProjectU / ProjectV
 * (ials.h:133-139, safer2.h:152-157, 210-215), there
 * Eigen::ConjugateGradient<MatrixXf, Lower> on the assembled d x d matrix:
 * here the same recurrence on the operator, A never formed (cg.hip),
 *   A p = s_G G p + sum_j c_j y_j (y_j . p) + lambda p
 * with the terms of frecsys_solve_side's assembly (IALS: s_G = w, c_j = 1;
 * WEIGHTED_U: s_G = omega w, c_j = omega / h; WEIGHTED_V: s_G = w, c_j = nu_j,
 * the parity tail-quirk rows a second time in c_j and not in b).  Recurrence
 * (Jacobi preconditioner, zero start):
 *   x = 0; r = b; ||b||^2 == 0 -> x = 0, 0 iterations
 *   thr = max(tolerance^2 ||b||^2, FLT_MIN); ||r||^2 < thr -> done
 *   p = r ./ diag(A); rho = r.p; i = 0
 *   while i < max_iterations:
 *     t = A p; alpha = rho / (p.t); x += alpha p; r -= alpha t
 *     if ||r||^2 < thr: break
 *     z = r ./ diag(A); rho' = r.z; p = z + (rho'/rho) p; rho = rho'; i += 1
 * (a zero diagonal entry has inverse 1): it stops at
 * ||r||^2 < tolerance^2 ||b||^2 or at i = max_iterations; max_iterations = 0
 * gives x = 0.  An entity's result bits do not depend on the other entities
 * of the call, the shard or the world size. */
typedef struct {
  int32_t max_iterations; /* --cg_max_iterations */
  float tolerance;        /* --cg_error_tolerance */
} frecsys_cg_params;
/* frecsys_solve_side by conjugate gradients: sides USER / ITEM / EVAL, kinds
 * IALS / WEIGHTED_U / WEIGHTED_V; the same sharding, all-gather of the rows,
 * external-exchange rules and "rows with an empty history are left
 * untouched".  FRECSYS_ERR_INVALID: max_iterations < 0, a negative or NaN
 * tolerance, a CVAR_GRAD kind (no CG form in the reference);
 * FRECSYS_ERR_UNSUPPORTED: dim > 256 (the CG kernel is built for dim <= 256);
 * FRECSYS_ERR_NAN: a non-finite result row (entity via
 * frecsys_last_error_entity); there is no NOT_SPD on this path.  Counters
 * "cg_iterations" (sum of i over the solved entities) and "cg_unconverged"
 * (entities that stopped at the cap); timer key "<solve>.cg";
 * frecsys_work("<solve>.cg"): sum_e i_e (2 d^2 + 4 h_e d) flops and
 * sum_e i_e (h_e d 4 + h_e 4) gather bytes. */
int frecsys_solve_side_cg(frecsys_ctx* ctx, int32_t side, const frecsys_solve_params* params,
                          const frecsys_cg_params* cg);
/* The i of the last frecsys_solve_side_cg per row of `side` (host [rows of
 * side]); -1 for a row not solved here (empty history, another rank's row, no
 * CG call yet). */
int frecsys_cg_iterations(frecsys_ctx* ctx, int32_t side, int32_t* host);
/* Per-user loss over `side` (USER or EVAL) rows against ITEM embeddings and
 * G[ITEM]: (1/h) sum (x.u - 1)^2 + beta u^T G u, halved if half != 0.
 * Rows with empty history get 0.  host_out [rows] may be NULL (result kept
 * on device); for USER it is gathered across ranks first.  Under external
 * exchange (world > 1, no communicator) nothing is gathered: a rank computes
 * the rows of its own shard and the other ranks' rows read 0. */
int frecsys_user_loss(frecsys_ctx* ctx, int32_t side, float beta, int32_t half,
                      float* host_out);
/* ---- iALS++ subspace solver (ialspp.h) ----
 * Rating index of every CSR entry of side USER or ITEM (the tuple's position
 * in the training file: the second member of the by_user / by_item pairs),
 * [nnz of side]; allocates the prediction vector of the training tuples.
 * EVAL rows use their CSR position as rating index. */
int frecsys_pp_set_rating_index(frecsys_ctx* ctx, int32_t side, const int32_t* rix);
/* PredictDataset (ialspp.h:480-520) over the rows of side USER (training
 * prediction vector) or EVAL (fold-in prediction vector):
 * pred[rating index] = item . user. */
int frecsys_pp_predict(frecsys_ctx* ctx, int32_t side);
/* One block Step of every row of `side` (USER, ITEM or EVAL) on columns
 * [start, end), end - start <= 128, against the other side's embeddings and
 * G[other]: params->kind IALS = iALS++ Step + ProjectBlock
 * (ialspp.h:351-424, 85-145; reg, reg_exp, unobserved_weight),
 * WEIGHTED_U / WEIGHTED_V = SAFER2++ StepU + ProjectU / StepV + ProjectV
 * (safer2pp.h:449-653, 97-216; entity_weight / entity_reg + other_weight +
 * alpha as for frecsys_solve_side, G[other] the omega-weighted Gramian for
 * WEIGHTED_V).  Updates the block of the rows and their predictions.
 * At world > 1 (USER / ITEM) each rank solves its own shard of the rows
 * (frecsys_shard_range).  With an in-call exchange -- RCCL, or the caller's
 * transport (frecsys_set_transport): one code path, only the transport call
 * differs -- the rows are then all-gathered, every rank replays the other
 * ranks' prediction updates from them, takes the same NOT_SPD verdict (a
 * min over ranks) and sums every rank's per-row residuals in the
 * single-rank order, so the embeddings, the prediction vector and the
 * residual are bitwise the single-rank ones.  Every rank must make the same
 * sequence of calls.  Without either (external exchange, no transport) the
 * caller copies the other ranks' rows in (frecsys_set_embeddings) and calls
 * frecsys_pp_sync -- also after a step that returned FRECSYS_ERR_NOT_SPD,
 * whose updates were applied; until it does, a further frecsys_pp_step or
 * frecsys_pp_predict on the context fails with FRECSYS_ERR_INVALID
 * ("pp_sync pending").  A step that fails for another reason leaves nothing
 * pending; its rows are then undefined (rerun frecsys_pp_predict).
 * residual (may be NULL): sum of squared block deltas (over every rank's
 * rows with an in-call exchange, this rank's rows otherwise). */
int frecsys_pp_step(frecsys_ctx* ctx, int32_t side, int32_t start, int32_t end,
                    const frecsys_solve_params* params, double* residual);
/* External-exchange completion of a sharded frecsys_pp_step on `side`: after
 * the other ranks' rows were set, apply their block updates to this rank's
 * prediction vector.  No reference counterpart (the sharded path is new). */
int frecsys_pp_sync(frecsys_ctx* ctx, int32_t side);
/* The prediction vector of the training tuples (side USER) or of the EVAL
 * rows (side EVAL), [nnz of the side] floats, indexed by rating index. */
int frecsys_pp_get_predictions(frecsys_ctx* ctx, int32_t side, float* host);
/* Caller-provided transport for the exchanges a sharded call makes inside
 * itself when the context has no RCCL communicator (frecsys_comm_init with
 * id NULL): the same points in the same order as the RCCL calls (today:
 * frecsys_pp_step).  Each callback returns 0 on success; every rank calls
 * them in the same order.
 *   allgather_rows: `rows` is a host copy of a whole per-row table of `side`
 *     (n_rows x ld floats, row-major); on entry rows [lo, hi) hold this
 *     rank's values, on return every row must hold its owner rank's values
 *     (an all-gather with the uneven counts of frecsys_shard_range);
 *   allreduce_min_u64: *value becomes the minimum over the ranks.
 * t == NULL removes the transport.  No reference counterpart. */
typedef struct frecsys_transport {
  void* user;
  int (*allgather_rows)(void* user, int32_t side, float* rows, int64_t n_rows, int64_t ld,
                        int64_t lo, int64_t hi);
  int (*allreduce_min_u64)(void* user, uint64_t* value);
} frecsys_transport;
int frecsys_set_transport(frecsys_ctx* ctx, const frecsys_transport* t);
/* Fold-in evaluation ranking (replaces the scoring + top-K of
 * EvaluateDatasetInternal / EvaluateUser, recommender.h:78-199): for every
 * row r of the EVAL side, scores s = V u_r over all items (fp32), the items
 * of row r's own EVAL history set to lowest() (the reference's `exclude`,
 * its fold-in history), then the k best items by descending score, ties by
 * ascending item id (the reference leaves tie order unspecified), into
 * topk[r*k .. r*k+k) (host int32).  1 <= k <= 1024, k <= items. */
int frecsys_eval_topk(frecsys_ctx* ctx, int32_t k, int32_t* topk);
/* Recommendations for rows of a user-factor table (no reference counterpart
 * beyond EvaluateUser's scoring, recommender.h:132-199): for each of the
 * n_rows query rows -- rows[i] of `side` (USER: the trained users, EVAL: the
 * fold-in rows; any order, repeats allowed), or rows 0 .. n_rows-1 when rows
 * is NULL -- the k best eligible items by descending score s = V u_r (each
 * score an fp32 FMA chain over the dim, the same whichever tile, item split
 * or row batch it falls in), ties by ascending item id, into
 * items[i*k .. i*k+k) and, unless scores is NULL, their scores into
 * scores[i*k .. i*k+k) (host).  An item is eligible when its item_mask byte
 * is non-zero (item_mask: host [n_items], or NULL = every item) and, with
 * FRECSYS_REC_EXCLUDE_HISTORY in flags, it is not in the CSR history of that
 * row on that side (USER: the training history, EVAL: the fold-in history).
 * 1 <= k <= 1024; k may exceed the eligible count: the slots beyond it hold
 * item -1 and score -FLT_MAX.  Scoring and top-K are fused on the device:
 * no rows x items score matrix exists; rows are ranked in batches whose
 * workspace (candidates, one history bitmap per row) stays within
 * FRECSYS_RECOMMEND_WS_MB (default 256), the items cut into
 * FRECSYS_RECOMMEND_SPLITS parts (default: enough for about 2 workgroups per
 * CU) -- neither changes a result bit.  Rank-local at any world size (every
 * rank holds the full tables after a step): no collective, no Gramian.
 * FRECSYS_ERR_INVALID: side ITEM, k out of range, a row id out of range, the
 * exclude flag on a side with no CSR loaded, null outputs.  Timer key
 * "recommend" (one launch per row batch); frecsys_work("recommend"):
 * 2 rows items d flops. */
#define FRECSYS_REC_EXCLUDE_HISTORY 1
int frecsys_recommend(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                      int32_t k, int32_t flags, const uint8_t* item_mask, int32_t* items,
                      float* scores);
/* Two-stage recommend: a bf16 retrieval scan picks a pool per row, the pool is
 * re-scored exactly, and a per-row certificate says when the list is
 * frecsys_recommend's bit for bit.  side, rows, item_mask, the exclude flag,
 * the eligibility and the outputs' layout are frecsys_recommend's;
 * 1 <= k <= pool <= 1024, pool = 0: min(1024, max(64, 4 k)).
 *
 * Notation: the query row r has the fp32 row x, item j the fp32 row y_j, Dp =
 * frecsys_padded_dim(dim), Dh = max(16, Dp) the width of the bf16 images.
 * Rounding: v^ = v rounded to bf16 by round-to-nearest-even; a NaN stays a NaN
 * (quiet); the exponent range is fp32's, so a finite value near FLT_MAX may
 * round to +-inf.  frecsys_bf16_round (host) is the definition -- it returns
 * the rounded values widened back to fp32 -- and the device conversion equals
 * it bit for bit.
 * Stage 1: s^_rj = the fp32 accumulator of v_mfma_f32_32x32x16_bf16 over x^_r
 * and y^_j from +0, the k-steps (16 columns each) in ascending order for every
 * (r, j), whatever the tile, split, batch or grid.  Row r's pool: its `pool`
 * best eligible items by (s^ descending, id ascending), built by
 * frecsys_recommend's candidate words, threshold rule and merge.  s^ is
 * defined to the bit against itself only, and bounded against float64 (below).
 * Stage 2: every pool item is re-scored as s_rj = frecsys_recommend's chain,
 * fmaf(y[c], x[c], acc), c ascending from +0; the list is the k best of the
 * pool by (s descending, id ascending), -1 / -FLT_MAX beyond the pool's fill.
 * Certificate: ||.|| = the Euclidean norm of the fp32 row, the squares summed
 * and the root taken in double on the device; N = max_j ||y_j|| over all item
 * rows; c(Dp) = 2^-7 + 2^-16 + 3 Dp 2^-23; B_r = c(Dp) ||x_r|| N in double
 * ((c ||x_r||) N; frecsys_two_stage_bound is the same arithmetic on the host).
 * (bf16 has unit roundoff u = 2^-8, so |x^y^ - xy| <= (2u + u^2)|xy|;
 * Cauchy-Schwarz bounds sum |x_c y_c| by ||x|| ||y||; frecsys_recommend's own
 * chain errs by about Dp 2^-24 sum |xy|; the matrix core's accumulation is
 * assumed to err by at most Dp 2^-23 sum |x^y^| -- together about 1.5 Dp 2^-23,
 * and the 3 is a 2x margin on the accumulation terms.)  certified[r] = 1 when
 *   (a) the pool is not full: every eligible item was re-scored; or
 *   (b) (double)s_k > (double)s^_P + B_r, strictly: s_k the k-th exact score of
 *       the list, s^_P the smallest approximate score of the full pool, and
 *       s_k, s^_P, B_r all finite.
 * Then every item outside the pool has s^ <= s^_P, so an exact score <= s^_P +
 * B_r < s_k, and the list is frecsys_recommend's bit for bit, ties included.
 * A row is never certified when the item table or its own query row holds a
 * value with 0 < |v^| < 2^-126 (the matrix core may flush subnormals).  For
 * every row, certified or not, every listed score is >= s*_k - 2 E_r, s*_k the
 * exact k-th best eligible score and E_r the row's largest |s^ - s|.
 * With FRECSYS_TS_EXACT in flags the uncertified rows are re-run through
 * frecsys_recommend's scan and their byte becomes 2: the outputs are then
 * frecsys_recommend's bits for EVERY row.
 * certified (host [n_rows], or NULL): 0 / 1 / 2.  pool_items / pool_scores
 * (host [n_rows * pool], or NULL): stage 1's pools as the scan left them, -1 /
 * -FLT_MAX beyond the fill.  The item image (items * Dh * 2 bytes) is rebuilt
 * by every call and released by frecsys_release_workspaces.  Rank-local.
 * FRECSYS_ERR_INVALID, before any device work: a bad side, k or pool, an
 * unknown flag, a row id out of range, null items with n_rows > 0, the exclude
 * flag without a CSR, a table without embeddings; n_rows == 0 returns
 * FRECSYS_OK.  Timer keys "two_stage.convert", "two_stage.scan",
 * "two_stage.select", "two_stage.fallback"; frecsys_work("two_stage.scan"):
 * 2 rows items d flops, (rows + items) Dh 2 + 8 rows pool bytes; counters
 * "two_stage_certified", "two_stage_fallback_rows". */
#define FRECSYS_TS_EXACT 2
int frecsys_recommend_two_stage(frecsys_ctx* ctx, int32_t side, const int64_t* rows,
                                int64_t n_rows, int32_t k, int32_t pool, int32_t flags,
                                const uint8_t* item_mask, int32_t* items, float* scores,
                                uint8_t* certified, int32_t* pool_items, float* pool_scores);
/* Host only, no context: out[i] = in[i] rounded to bf16 (see above), as fp32. */
int frecsys_bf16_round(const float* in, int64_t n, float* out);
/* Host only: B = c(Dp) * query_norm * item_norm_max in double, Dp =
 * frecsys_padded_dim(dim); NaN for an unsupported dim. */
double frecsys_two_stage_bound(int32_t dim, double query_norm, double item_norm_max);
/* Recall@K and NDCG@K of ranked lists on the host: the reference's
 * RankMetrics (recommender.h:152-182), once for every caller.  No context and
 * no HIP call: works on a machine without a GPU, like frecsys_partition.
 * Row i has the ranked list lists[i*list_k .. i*list_k+list_k) (-1: an empty
 * slot, never a hit) and the ground truth = the DISTINCT ids of
 * gt_items[gt_ptr[i] .. gt_ptr[i+1]), g of them.  For cut-off k = k_list[q]:
 * hits and dcg are double sums over the positions j < min(k, list_k) in
 * ascending j (dcg adds 1.0 / log2(j + 2.0)), norm the double sum of the same
 * terms for j < min(k, g), recall[i*nk+q] = (float)(hits / min((float)k,
 * (float)g)), ndcg[i*nk+q] = (float)(dcg / norm).  1 <= nk <= 32,
 * 1 <= k_list[q] <= 1024, any order, repeats allowed.  FRECSYS_ERR_INVALID: a
 * null pointer, gt_ptr[0] != 0 or a non-monotone gt_ptr, a negative
 * ground-truth id, a row with no ground truth (the reference's eval_by_user
 * holds none; 0 / 0 would poison the CVaR sort), list_k < max k_list. */
int frecsys_list_metrics(const int32_t* lists, int64_t n, int32_t list_k, const int64_t* gt_ptr,
                         const int32_t* gt_items, const int32_t* k_list, int32_t nk,
                         float* recall, float* ndcg);
/* Lower-tail CVaR of n per-user metric values at each of na alphas:
 * EvaluationResult::cvar (evaluation.h:83-102) verbatim, host only.  The
 * values are sorted ascending and summed sequentially in fp32; at sorted
 * position i, for j = counter .. na-1: where (int)((float)n * alphas[j]) == i,
 * out[counter++] = sum / (float)(i + 1).  The reference's quirks follow and
 * stay: results fill out[] in match order, not at index j; an alpha whose
 * position is >= n (alpha = 1) leaves its slot 0; with unsorted alphas the
 * later slots stay 0.  out: [na]. */
int frecsys_metric_cvar(const float* values, int64_t n, const float* alphas, int32_t na,
                        float* out);
/* Evaluation on the device: frecsys_list_metrics of frecsys_recommend's
 * ranking with k = max(k_list), bitwise, without the lists leaving the
 * device.  side, rows, flags and item_mask mean what they mean for
 * frecsys_recommend; ground-truth row i (gt_items[gt_ptr[i] .. gt_ptr[i+1]))
 * belongs to query row i (not to side row rows[i]); recall, ndcg: host
 * [n_rows * nk].  An excluded or masked item is never listed, so never a hit.
 * Per row batch the fused scan of frecsys_recommend runs, then one kernel
 * (one wave per row: binary search of each rank in the row's sorted distinct
 * ground truth, one ballot per 64 ranks, one lane per cut-off) reads the lists
 * where the scan left them, and 2 nk floats per row are copied back.  Equality
 * with the host function holds because every device operation is an IEEE
 * double add, divide or convert on the host's own operands (the 1/log2 terms
 * and their prefix sums are uploaded from the host) in the host's order.
 * Workspace: frecsys_recommend's, the batch sized by FRECSYS_RECOMMEND_WS_MB
 * with 8 nk more bytes per row, and outside that budget 8 (n_rows + 1) +
 * 4 (ground-truth ids) + 16,392 (tables) + 4 nk bytes: the ground truth,
 * sorted and de-duplicated per row on host threads while the first batch is
 * scanned, and uploaded once per call.  FRECSYS_RECOMMEND_WS_MB / _SPLITS are read per call and change no
 * result bit.  Rank-local at any world size.  FRECSYS_ERR_INVALID:
 * frecsys_recommend's cases, frecsys_list_metrics' cases, a ground-truth id
 * >= n_items.  Timer key "rank_metrics": the metric kernel only (the scan
 * keeps "recommend"); frecsys_work("rank_metrics"): 2 rows nk flops (the
 * divisions), bytes = lists and ground truth read, metric rows written. */
int frecsys_rank_metrics(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                         int32_t flags, const uint8_t* item_mask, const int64_t* gt_ptr,
                         const int32_t* gt_items, const int32_t* k_list, int32_t nk,
                         float* recall, float* ndcg);
/* MRR and AUC of full-catalogue positions on the host (no reference
 * counterpart; the expected-percentile-rank family of the original iALS
 * evaluation).  No context and no HIP call, like frecsys_list_metrics.  Row i
 * has the positions rank[gt_ptr[i] .. gt_ptr[i+1]) of its ground-truth entries
 * (frecsys_rank_positions: 0-based, -1 = the item is not eligible) among
 * M = eligible[i] eligible items.  R = the ascending distinct non-negative
 * ranks of the row, g = |R| (distinct items have distinct ranks).  mrr[i] =
 * g ? (float)(1.0 / (double)(R[0] + 1)) : 0.0f.  auc[i] = 0.0f when g = 0,
 * 1.0f when M = g, else (float)(1.0 - (double)inv / ((double)g * (double)(M -
 * g))) with inv = sum_q (R[q] - q) as an int64: the number of (held-out, other
 * eligible) pairs in the wrong order -- an integer, so no summation order has
 * to be stated.  mrr, auc: [n_rows].  FRECSYS_ERR_INVALID: a null pointer,
 * n_rows < 0, gt_ptr[0] != 0 or a non-monotone gt_ptr, a row with no ground
 * truth (as for frecsys_list_metrics; a row whose ground truth is entirely
 * ineligible is valid and scores 0 / 0), a rank outside [-1, eligible[i]).  All
 * checks come before the first write. */
int frecsys_position_metrics(const int32_t* rank, const int64_t* gt_ptr, const int32_t* eligible,
                             int64_t n_rows, float* mrr, float* auc);
/* Exact positions of ground-truth items in the full ranking (no reference
 * counterpart): what frecsys_recommend cannot report past k = 1024.  side,
 * rows, flags and item_mask mean what they mean for frecsys_recommend;
 * ground-truth row i (gt_items[gt_ptr[i] .. gt_ptr[i+1]), not empty, repeats
 * allowed) belongs to query row i.  E_i = the eligible items of row i as
 * frecsys_recommend defines them, word(i, j) = (u64)score_key(s_ij) << 32 |
 * ~(u32)j with s_ij frecsys_recommend's score bit for bit.  For entry t with
 * item j: rank[t] = -1 when j is not in E_i, else the number of j' in E_i with
 * word(i, j') > word(i, j) -- the 0-based slot frecsys_recommend would list j
 * in if its k were large enough; ties by ascending item id; a repeated id has
 * the same rank at every occurrence.  eligible[i] = |E_i|.  mrr / auc are
 * frecsys_position_metrics of those ranks, bitwise, computed on the device
 * without the ranks leaving it.  rank: host [gt_ptr[n_rows]]; eligible, mrr,
 * auc: host [n_rows]; each may be NULL, not all four.
 * Per row batch: the history bits as for frecsys_recommend; one kernel scores
 * every ground-truth entry by frecsys_score_pairs' chain (the scan's bits),
 * forms the words and sorts each row's distinct eligible ones descending as
 * thresholds; the scan (frecsys_recommend's tile and FMA chain; no score
 * matrix, no candidate buffers, no top-K) counts, per row, the eligible items
 * between consecutive thresholds with integer atomics (rows with up to 32
 * thresholds in LDS, longer ones in global memory, as exactly); one wave per
 * row turns the counts into ranks by a prefix sum, counts the eligibility
 * bits, and forms mrr / auc with the host function's own int64 and IEEE
 * double operations.  Workspace: per batch 28 bytes per ground-truth entry and
 * 20 per row plus the history bits, the rows cut greedily so that a batch
 * stays within FRECSYS_RECOMMEND_WS_MB (at least one row); the items are cut
 * into FRECSYS_RECOMMEND_SPLITS parts as for frecsys_recommend.  Both knobs
 * are read per call and change no result bit.  Rank-local at any world size.
 * n_rows == 0 returns FRECSYS_OK and touches nothing.  FRECSYS_ERR_INVALID,
 * before any device call: frecsys_recommend's cases but k, the ground-truth
 * cases of frecsys_rank_metrics (a ground-truth id >= n_items among them),
 * all four outputs NULL.  Timer key "rank_positions" (one launch group per
 * row batch; nothing runs under "recommend"); frecsys_work("rank_positions"):
 * 2 rows items d flops, bytes = the ground truth read, the ranks and the
 * three values per row written. */
int frecsys_rank_positions(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                           int32_t flags, const uint8_t* item_mask, const int64_t* gt_ptr,
                           const int32_t* gt_items, int32_t* rank, int32_t* eligible, float* mrr,
                           float* auc);
/* Scores of caller-supplied pairs (no reference counterpart): scores[i] =
 * V[items[i]] . X[rows[i]] for the n_pairs pairs, X the table of `side` (USER
 * or EVAL), rows / items / scores host arrays [n_pairs]; any order, repeats
 * allowed.  A score is bit for bit the one frecsys_recommend lists for that
 * row and item: the fp32 chain acc = fma(v[c], x[c], acc) over the padded dim
 * in ascending c from +0 (pad columns add +0; never -0.0), whatever the pair's
 * position, the batch, or whether frecsys_rank_candidates computed it.  One
 * wave per 64 pairs gathers both rows in 32-column slabs through LDS; pairs
 * are scored in batches whose workspace (16 bytes per pair: ids and score)
 * stays within FRECSYS_RECOMMEND_WS_MB (default 256), which changes no result
 * bit.  Rank-local at any world size: no collective.  n_pairs == 0 returns
 * FRECSYS_OK and touches nothing.  FRECSYS_ERR_INVALID, before any device
 * call: a null context, side ITEM, a null pointer, a row id or an item id out
 * of range.  Timer key "score_pairs" (one launch per batch);
 * frecsys_work("score_pairs"): 2 pairs d flops, bytes = pairs Dp 4 (one padded
 * item row per pair) + 12 pairs (ids) + 4 pairs (scores). */
int frecsys_score_pairs(frecsys_ctx* ctx, int32_t side, const int64_t* rows,
                        const int32_t* items, int64_t n_pairs, float* scores);
/* Explanations (no reference counterpart): a score split exactly over the
 * history entries of a row.  The projection frecsys_solve_side computes for
 * `params` (kinds IALS and WEIGHTED_U) solves A x = b with
 *   A = s_G G + sum_j c_j y_j y_j^T + lambda I,   b = sum_j c_j y_j
 * over the history rows y_j of the row (s_G, c_j, lambda per kind as tabulated
 * at frecsys_solve_side_cg), so the score of an item t is
 *   v_t . x = sum_j contrib_j(t),   contrib_j(t) = c_j y_j^T A^-1 v_t.
 * Query row i -- CSR row rows[i] of `side` (USER or EVAL), or row i when rows
 * is NULL -- is explained for its targets tgt_items[tgt_ptr[i] ..
 * tgt_ptr[i+1]); pairs are numbered in that order.  Solved against the ITEM
 * table and G[ITEM] as the context holds them (frecsys_solve_side's contract
 * on those sides; from_snapshot is ignored); the embeddings of `side` are
 * neither read nor written.  Repeated rows and targets are allowed, every pair
 * is independent.  score: [pairs], the sum of the pair's contributions (lane l
 * of a wave adds the entries l, l + 64, ... in CSR order, then a fixed
 * butterfly over the 64 partial sums) -- the score of the exact projection of
 * that history against the current item table, not U[row] . V[t].  top_items /
 * top_contrib: [pairs * top], the `top` (1..32) largest contributions by
 * (contribution descending, CSR position ascending) with their history item
 * ids, -1 / 0 behind the row's history length; a row with an empty history
 * has score 0 and only fill.  full: NULL, or the h contributions of every pair
 * in CSR order, pairs in order (sum over pairs of their row's h floats).  The
 * bits of a pair depend on the row's history, the parameters and the tables
 * only -- not on the batch, the other rows or targets, their grouping, `top`,
 * FRECSYS_RECOMMEND_WS_MB or the side.  Rank-local at any world size: no
 * collective.  Zero rows or zero targets return FRECSYS_OK without a launch.
 * FRECSYS_ERR_INVALID, before any device call: a null context, side ITEM, a
 * kind other than IALS / WEIGHTED_U, top out of range, a null pointer, no CSR
 * on the side, a row id or target id out of range, tgt_ptr not starting at 0
 * or not monotone.  FRECSYS_ERR_UNSUPPORTED: dim > 256.  FRECSYS_ERR_NOT_SPD:
 * a failed pivot (entity via frecsys_last_error_entity).  Timer key "explain"
 * (one launch group per batch); frecsys_work("explain"): per row with h
 * entries and m targets h d^2 + d^3 / 3 + 2 d^2 m + 2 h d m flops, bytes = the
 * history rows gathered (once to assemble, once per 32 targets) + the target
 * rows. */
int frecsys_explain(frecsys_ctx* ctx, int32_t side, const frecsys_solve_params* params,
                    const int64_t* rows, int64_t n_rows, const int64_t* tgt_ptr,
                    const int32_t* tgt_items, int32_t top, float* score, int32_t* top_items,
                    float* top_contrib, float* full);
/* Host-only: lengths[i] = the history length of CSR row rows[i] of `side` (row
 * i when rows is NULL) as loaded -- what sizes frecsys_explain's `full`.
 * FRECSYS_ERR_INVALID: no CSR on the side, a row id out of range. */
int frecsys_csr_row_lengths(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                            int64_t* lengths);
/* Ranking of caller-supplied candidate lists (the second stage of a
 * retrieve-then-rank pipeline; no reference counterpart): query row i --
 * rows[i] of `side`, or row i when rows is NULL -- ranks the DISTINCT eligible
 * ids of its own list cand_items[cand_ptr[i] .. cand_ptr[i+1]) (list i belongs
 * to query row i, as gt_ptr does in frecsys_rank_metrics; any length, 0 and
 * more than n_items included; any order, repeats allowed and counted once).
 * side, rows, flags (FRECSYS_REC_EXCLUDE_HISTORY), item_mask, the order (score
 * descending, ties by ascending item id), the outputs items / scores
 * [n_rows * k] (scores may be NULL) and the -1 / -FLT_MAX fill beyond the
 * eligible distinct count mean what they mean for frecsys_recommend, and every
 * score is that function's bit for bit (the chain of frecsys_score_pairs).
 * 1 <= k <= 1024.  One workgroup per query row keeps the row of X in LDS,
 * gathers the list in chunks of 256 item rows, and keeps at most 2048
 * candidate words (score key << 32 | ~id) in LDS, sorted and cut to the best
 * k distinct before a chunk might not fit; once k are known a candidate below
 * the k-th key is dropped, one that ties it is kept (a list is in no id
 * order).  Rows are ranked in batches (cut in row order, at least one row
 * each) whose workspace -- 4 bytes per candidate id, 8 k bytes of outputs and,
 * with the exclude flag, 4 * 4 * ceil(n_items / 128) bytes of history bits per
 * row -- stays within FRECSYS_RECOMMEND_WS_MB (default 256); outside that
 * budget lie 8 (n_rows + 1) bytes of cand_ptr, 8 n_rows of row ids and the
 * mask bits.  The knob changes no result bit.  Rank-local at any world size:
 * no collective.  n_rows == 0 returns FRECSYS_OK and touches nothing.
 * FRECSYS_ERR_INVALID, before any device call: a null context, side ITEM, k
 * out of range, an unknown flag, a row id out of range, a null cand_ptr /
 * items (cand_items too unless every list is empty), cand_ptr[0] != 0 or a
 * non-monotone cand_ptr, a candidate id < 0 or >= n_items, the exclude flag on
 * a side with no CSR loaded.  Timer key "rank_candidates" (one launch group
 * per row batch); frecsys_work("rank_candidates"): 2 pairs d flops with
 * pairs = cand_ptr[n_rows], bytes = pairs Dp 4 + 4 pairs (ids) + 8 k n_rows
 * (lists). */
int frecsys_rank_candidates(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                            const int64_t* cand_ptr, const int32_t* cand_items, int32_t k,
                            int32_t flags, const uint8_t* item_mask, int32_t* items,
                            float* scores);
/* Metrics of candidate lists on the device (second-stage evaluation; no
 * reference counterpart): frecsys_list_metrics(L, list_k = k, gt, k_list) of
 * the lists L that frecsys_rank_candidates returns with k = max(k_list) and
 * the same side, rows, cand_ptr / cand_items, flags and item_mask -- bitwise,
 * without the lists leaving the device.  Ground-truth row i belongs to query
 * row i; a ground-truth id that is not in the list, is masked out or is
 * excluded as history is simply never a hit, and g stays the count of
 * distinct ground-truth ids.  Per row batch rank_cand_kernel ranks the
 * uploaded lists and frecsys_rank_metrics' kernel reads the top-K where the
 * ranking left it; 2 nk floats per row come back (recall, ndcg: host
 * [n_rows * nk]).  Batches are frecsys_rank_candidates' (4 bytes per id, 4 k +
 * 8 nk bytes of outputs and the history bits per row within
 * FRECSYS_RECOMMEND_WS_MB, which changes no result bit); the ground truth,
 * tables and cut-offs lie outside that budget as for frecsys_rank_metrics.
 * Rank-local at any world size: no collective.  n_rows == 0 returns
 * FRECSYS_OK and touches nothing.  FRECSYS_ERR_INVALID, before any device
 * call: frecsys_rank_candidates' cases and frecsys_rank_metrics' cases.
 * Timer keys "rank_candidates" and "rank_metrics", with their work
 * definitions (the lists written count 4 k bytes per row: no scores). */
int frecsys_rank_candidates_metrics(frecsys_ctx* ctx, int32_t side, const int64_t* rows,
                                    int64_t n_rows, const int64_t* cand_ptr,
                                    const int32_t* cand_items, int32_t flags,
                                    const uint8_t* item_mask, const int64_t* gt_ptr,
                                    const int32_t* gt_items, const int32_t* k_list, int32_t nk,
                                    float* recall, float* ndcg);
/* The negatives of sampled evaluation, on the host (no context, no HIP call,
 * like frecsys_list_metrics): what frecsys_sampled_metrics draws on the
 * device, bit for bit.  For query row i with side row id r = row_ids[i] (i
 * when row_ids is NULL), history hist_items[hist_ptr[i] .. hist_ptr[i+1])
 * (per QUERY row; both NULL = no exclusion; ids outside [0, n_items) are
 * ignored) and ground truth gt_items[gt_ptr[i] .. gt_ptr[i+1]):
 *   D = the ascending ids whose item_mask byte is non-zero (all of
 *   0 .. n_items-1 when item_mask is NULL), M = |D|;
 *   pool = { j in D : j not in the ground truth, j not in the history },
 *   E = |pool|.
 * Whole-pool row (2 n_neg > E or 64 E < M): the negatives are all of pool,
 * neg_count[i] = E, and negatives[i*n_neg ..) is filled with -1 (the ids are
 * not returned).  This bounds the expected draws of every other row by
 * 128 n_neg.  Sampled row otherwise: with mix64(x) = splitmix64's finaliser
 * (x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 * x *= 0x94D049BB133111EB; x ^= x >> 31) and C = 0x9E3779B97F4A7C15, all in
 * wrapping uint64: key = mix64(seed + C (r + 1)); for t = 0, 1, ...:
 * u = mix64(key + C (t + 1)), idx = ((u >> 32) M) >> 32, j = D[idx]; draw t
 * is accepted when j is in pool and differs from every accepted earlier
 * draw; the negatives are the first n_neg accepted draws in draw order,
 * neg_count[i] = n_neg.  A row's sample depends on (seed, r, n_neg, mask,
 * its ground truth, its history) only -- not on the other rows of the call,
 * the batch, the grid or the world size.  A row stops after 2^20 + 4096 n_neg
 * draws at the latest (never reached in practice: a draw is accepted with
 * probability >= 1/128) and the call then fails with FRECSYS_ERR_HIP, the
 * code of the device call with the same cap.  Rows run on the host thread
 * pool.  neg_count: [n_rows]; negatives: [n_rows * n_neg] or NULL.
 * n_rows == 0 returns FRECSYS_OK and touches nothing.  FRECSYS_ERR_INVALID,
 * outputs untouched: n_items outside [1, 2^31), n_rows < 0, n_neg < 0,
 * n_rows * n_neg overflowing int64, a negative row id, null neg_count / gt_ptr
 * / gt_items, hist_items without hist_ptr (or the reverse with a non-empty
 * history), a negative or non-monotone hist_ptr, gt_ptr[0] != 0 or a
 * non-monotone gt_ptr, a row with no ground truth, a ground-truth id outside
 * [0, n_items). */
int frecsys_sample_negatives(int64_t n_items, const uint8_t* item_mask, const int64_t* row_ids,
                             int64_t n_rows, const int64_t* hist_ptr, const int32_t* hist_items,
                             const int64_t* gt_ptr, const int32_t* gt_items, int32_t n_neg,
                             uint64_t seed, int32_t* neg_count, int32_t* negatives);
/* Sampled evaluation on the device: frecsys_rank_candidates_metrics of the
 * lists cand_i = distinct(gt_i) followed by the negatives
 * frecsys_sample_negatives defines for (n_items, item_mask, r = rows[i],
 * history = the CSR history of row r of `side` when flags has
 * FRECSYS_REC_EXCLUDE_HISTORY, else none) -- for a whole-pool row all of its
 * pool.  Every ground-truth id is in the list, eligible or not; the ranking
 * drops the ineligible ones as it always does.  When every row is a
 * whole-pool row (n_neg >= n_items, say) the result is frecsys_rank_metrics'
 * bitwise.  Sampled metrics are NOT estimates of the full-catalogue metrics
 * of frecsys_rank_metrics and must not be read as such: they rank systems
 * differently (Krichene & Rendle, KDD 2020).
 *   Per row batch: one bitmap per row (the layout of the other paths,
 * 16 ceil(n_items / 128) bytes) receives the blocked bits (history and ground
 * truth), one pass counts E, and 4 bytes per row come back so that the host
 * lays the lists out; one wave per row then writes its list into the buffer
 * rank_cand_kernel reads -- a sampled row in blocks of 64 draws (lane l holds
 * draw t0 + l; a 64-bit ballot orders the accepted lanes; taken ids are
 * marked in the row's bitmap), a whole-pool row by compacting its eligible
 * bits -- and the ranking and the metric kernel follow.  Only 2 nk floats per
 * row come back, plus neg_count [n_rows] and negatives [n_rows * n_neg] (as
 * frecsys_sample_negatives returns them) where those are not NULL.
 * Workspace: rows are cut into batches whose bitmaps and outputs (16
 * ceil(n_items / 128) + 4 k + 8 nk bytes per row) stay within half of
 * FRECSYS_RECOMMEND_WS_MB (default 256), each batch into sub-batches whose
 * lists (4 (g_i + neg_count_i) bytes per row, from the counted pools) stay
 * within the other half, at least one row each; outside that budget lie 20
 * bytes per row (list offsets, row ids, pool counts), the ground truth and
 * tables of frecsys_rank_metrics, the mask bits and 4 M bytes of D when a
 * mask is given.  The knob changes no result bit.  All of it goes with
 * frecsys_release_workspaces.  Rank-local at any world size: no collective.
 * n_rows == 0 returns FRECSYS_OK and touches nothing.  FRECSYS_ERR_INVALID,
 * before any device call: frecsys_rank_candidates' and frecsys_rank_metrics'
 * cases, n_neg < 0, n_rows * n_neg overflowing int64.  FRECSYS_ERR_HIP: a row
 * reached the draw cap of frecsys_sample_negatives (the kernel loop stops
 * there and raises the context's fail word; it never hangs).  Timer keys
 * "sample_negatives" (the bitmap, pool and list kernels), "rank_candidates"
 * and "rank_metrics"; frecsys_work("sample_negatives"): 0 flops, bytes =
 * 2 x 16 ceil(n_items / 128) per row (its bitmap written, then read by the
 * pool pass) + 4 per list id written. */
int frecsys_sampled_metrics(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                            int32_t flags, const uint8_t* item_mask, const int64_t* gt_ptr,
                            const int32_t* gt_items, int32_t n_neg, uint64_t seed,
                            const int32_t* k_list, int32_t nk, float* recall, float* ndcg,
                            int32_t* neg_count, int32_t* negatives);
/* Nearest neighbours inside one factor table ("items like this item", "users
 * like this user"; no reference counterpart): T, the table of `side` (USER or
 * ITEM), is both the source of the queries and the table searched.  Query row
 * i is row rows[i] of T (any order, repeats allowed), or row i when rows is
 * NULL; it lists the k best eligible rows of T by descending score, ties by
 * ascending id, into ids[i*k .. i*k+k) and, unless scores is NULL, their
 * scores into scores[i*k .. i*k+k) (host).  A row j is eligible when its mask
 * byte is non-zero (mask: host [rows of side], or NULL = every row) and,
 * without FRECSYS_SIM_KEEP_SELF, j != rows[i]: a query never lists its own id,
 * but rows that are equal to it in value are listed (cosine ~ 1, ties by id).
 * 1 <= k <= 1024; the slots beyond the eligible count hold id -1 and score
 * -FLT_MAX, as in frecsys_recommend.
 *   dot(q, j): frecsys_recommend's chain, acc = fma(T[j][c], T[q][c], acc)
 * over the padded dim in ascending c from +0 -- bit for bit what
 * frecsys_recommend would list if T were both its user and its item table.
 * Without FRECSYS_SIM_COSINE it is the score.
 *   With FRECSYS_SIM_COSINE: n2_r = dot(r, r), inv_r = n2_r > 0 ?
 * 1.0f / sqrtf(n2_r) : 0.0f with correctly rounded sqrt and division, and the
 * score is (dot(q, j) * inv_q) * inv_j + 0.0f, two fp32 multiplies in exactly
 * that order (the + 0.0f keeps -0.0 out of the keys, as the dot chain does by
 * construction).  A zero row has cosine +0 with everything.  inv_r depends on
 * row r alone, not on the batch, the split or the grid.
 * The norms are computed per call (one lane per row, the chain above: the
 * tables change with every solve), the scan is frecsys_recommend's with the
 * scores scaled before they become keys and the row's own id cleared from its
 * eligibility bits; no normalised copy of T and no rows x rows score matrix
 * exists.  Workspace and knobs are frecsys_recommend's (FRECSYS_RECOMMEND_WS_MB,
 * FRECSYS_RECOMMEND_SPLITS: read per call, neither changes a result bit), no
 * history bitmap; the inverse norms add 4 * rows-of-side bytes outside the
 * per-row budget.  Both buffers go with frecsys_release_workspaces.
 * Rank-local at any world size: no collective.  n_rows == 0 returns
 * FRECSYS_OK and touches nothing.  FRECSYS_ERR_INVALID, before any device
 * call: a null context, side EVAL or unknown, k out of range, an unknown flag
 * bit, a row id out of range, rows == NULL with n_rows above the side's rows,
 * null ids with n_rows > 0, a side without embeddings.  Timer keys "similar"
 * (one launch group per row batch) and "similar.norms";
 * frecsys_work("similar"): 2 rows m d flops (m = rows of side), bytes =
 * (rows + 2 m) d 4 + 8 rows k (the second m d 4 is the norm pass: cosine
 * only). */
#define FRECSYS_SIM_COSINE 1    /* score = cosine; without it: dot product */
#define FRECSYS_SIM_KEEP_SELF 2 /* without it a query row never lists itself */
int frecsys_similar(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                    int32_t k, int32_t flags, const uint8_t* mask, int32_t* ids, float* scores);
/* Audiences: the k best users for items ("who should see this item?"; the
 * reference has no counterpart, Spark's ALS calls it recommendForItemSubset).
 * Query i is row items[i] of the ITEM table (any order, repeats allowed), or
 * row i when items is NULL; it lists the k best eligible users by descending
 * score, ties by ascending user id, into users[i*k .. i*k+k) and, unless
 * scores is NULL, their scores into scores[i*k .. i*k+k) (host).
 *   score(i, u): acc = fma(V[i][c], U[u][c], acc) over the padded dim in
 * ascending c from +0 -- bit for bit frecsys_score_pairs(USER, u, i) and the
 * score frecsys_recommend lists for item i in user u's row (the product
 * commutes, the order of c is the same, and a chain from +0 never yields -0).
 *   A user u is eligible when its user_mask byte is non-zero (host [users],
 * or NULL = every user) and, with FRECSYS_AUD_EXCLUDE_HISTORY, u is not in
 * the ITEM-side CSR row of the query item (the users who interacted with it;
 * columns unsorted, repeats allowed).  1 <= k <= 1024; the slots beyond the
 * eligible count hold id -1 and score -FLT_MAX.
 *   Two paths, one result.  n <= FRECSYS_AUDIENCE_THIN_MAX (read per call;
 * default 4096, 0 forces the scan) takes the thin-query kernel (audience.hip):
 * 8 queries stay on chip while a workgroup sweeps its split of the user table
 * once per pass, and the splits' lists are merged in rounds.  More queries
 * take frecsys_recommend's scan with the item rows as queries and the user
 * table searched.  frecsys_audience_plan answers what is launched.  Neither
 * the path, the splits, the passes nor the batch changes a result bit; no
 * rows x users score matrix exists.  Workspace and knobs are
 * frecsys_recommend's (FRECSYS_RECOMMEND_WS_MB, FRECSYS_RECOMMEND_SPLITS), the
 * workspace goes with frecsys_release_workspaces.  Rank-local at any world
 * size: no collective.  n == 0 returns FRECSYS_OK and touches nothing.
 * FRECSYS_ERR_INVALID, before any device call: a null context, k out of range,
 * an unknown flag bit, an item id out of range, items == NULL with n above
 * the item count, null users with n > 0, the exclude flag without an ITEM CSR
 * loaded, a table without embeddings, no users.  Timer key "audience": one
 * launch group per query batch, the table passes of a batch in one grid;
 * frecsys_work("audience"): 2 n m d flops (m = users), bytes = (passes m + n)
 * Dp 4 + 8 n k with the plan's passes. */
#define FRECSYS_AUD_EXCLUDE_HISTORY 1
int frecsys_audience(frecsys_ctx* ctx, const int64_t* items, int64_t n, int32_t k,
                     int32_t flags, const uint8_t* user_mask, int32_t* users, float* scores);
/* What frecsys_audience launches for n queries against n_users users on a
 * device of `cus` compute units (host arithmetic only: no context, no HIP
 * call; reads the three knobs above as the call does).
 *   thin: 1 = the thin-query kernel, 0 = the scan.  queries_per_pass: queries
 * that share one read of the table (thin: 8, fewer when the budget holds
 * fewer; scan: its 64-row block); passes = ceil(n / queries_per_pass).
 * splits: the table is swept in chunks of chunk_rows rows; with C =
 * ceil(n_users / chunk_rows), split s takes chunks [s C / splits, (s + 1) C /
 * splits).  slots: candidate words per (query, split), >= k + chunk_rows.
 * merge_rounds: the kernels behind the scan -- on the thin path every round
 * but the last takes the k best of groups of 8192 / kp lists (kp: k rounded up
 * to a power of two, 64 at least) and the last writes out the one list left;
 * the scan's one merge takes its splits, at most 8192 / k.  rows_per_batch: queries per launch group;
 * workspace_bytes: what a batch takes of the budget.  FRECSYS_ERR_INVALID: an
 * unsupported dim, n_users < 1, n < 1, k outside [1, 1024], cus < 1, exclude
 * not 0 / 1, a null out. */
typedef struct {
  int32_t thin, queries_per_pass, passes, splits, chunk_rows, slots, merge_rounds;
  int64_t rows_per_batch, workspace_bytes;
} frecsys_audience_plan_t;
int frecsys_audience_plan(int32_t dim, int64_t n_users, int64_t n, int32_t k, int32_t cus,
                          int32_t exclude, frecsys_audience_plan_t* out);
/* Diversified lists: greedy maximal-marginal-relevance (MMR) re-ranking of a
 * pool of items per query row (no reference counterpart).  The three calls
 * below share one definition, fixed to the bit; frecsys_mmr_select is that
 * definition in scalar C++ on the host, and the two device calls return its
 * bits.
 *   Pool.  A row has `pool` slots (1 <= k <= pool <= 1024) of an item id and
 * an fp32 score.  A slot with a negative id is empty; ids may repeat, and each
 * slot is a candidate of its own.  p = the number of filled slots.
 *   Relevance.  With FRECSYS_DIV_RAW_SCORES rel_b = score_b.  Otherwise smax
 * and smin are the largest and smallest score of the filled slots, range =
 * smax - smin, and rel_b = range > 0 ? (score_b - smin) / range : 0.0f; the
 * subtractions and the division are single correctly rounded fp32 operations.
 *   Similarity of slot a (already selected) and slot b (a candidate), over
 * the item table Y: g = dot(Y[id_a], Y[id_b]) is frecsys_similar's chain, acc
 * = fma(Y[id_a][c], Y[id_b][c], acc) over c ascending from +0; n2_r =
 * dot(r, r); inv_r = n2_r > 0 ? 1.0f / sqrtf(n2_r) : 0.0f with correctly
 * rounded sqrt and division; cos(a, b) = (g * inv_a) * inv_b + 0.0f, the two
 * fp32 multiplies in exactly that order.  A zero item row has cosine +0 with
 * everything.
 *   Greedy selection.  lam is in [0, 1], oml = 1.0f - lam, base_b = lam *
 * rel_b.  Step 0: v_b = base_b + 0.0f.  Step t >= 1: m_b = fmaxf over the
 * selected slots s_u, u < t, of cos(s_u, b) (m_b may be negative: it is not
 * clamped at 0), and v_b = (base_b - oml * m_b) + 0.0f -- a separate fp32
 * multiply and subtraction, never contracted into an fma.  s_t is the
 * unselected filled slot with the largest word score_key(v_b) << 32 | ~b
 * (score_key: the order-preserving map of the fp32 bits to uint32): the
 * largest v, ties to the lower slot -- in a pool from frecsys_recommend that
 * is the higher score, then the lower id.
 *   Outputs (host), per row and t < k: items[t] = the id of s_t, scores[t] =
 * its pool score with its bits unchanged, and, unless mmr is NULL, mmr[t] = v
 * at its selection.  For t >= p: -1, -FLT_MAX and -FLT_MAX.  No output ever
 * holds -0.0 in mmr.  At lam = 1 the selection is the first k slots of the
 * pool in (score descending, slot ascending) order.
 * No output bit depends on the batch, the grid, the workspace budget, the
 * item splits, the other rows, or how the pool reached the device.
 * FRECSYS_ERR_INVALID for all three: pool outside [1, 1024], k outside
 * [1, pool], lam outside [0, 1] or NaN, an unknown flag bit, a negative row
 * count, null outputs (items, scores) with rows > 0.  Zero rows return
 * FRECSYS_OK and touch nothing.
 *
 * frecsys_mmr_select: host only -- no context, no HIP call.  item_table is
 * row-major [n_items][ld] with ld >= dim >= 1; lists / list_scores are
 * [n][pool]; items / scores / mmr are [n][k].  Also FRECSYS_ERR_INVALID: a
 * null table or pool array, an id >= n_items, a non-finite score in a filled
 * slot, and (without FRECSYS_DIV_RAW_SCORES) a non-finite range. */
#define FRECSYS_DIV_RAW_SCORES 2 /* rel = the pool score; without it: min-max normalised */
int frecsys_mmr_select(const float* item_table, int64_t n_items, int32_t dim, int64_t ld,
                       const int32_t* lists, const float* list_scores, int64_t n, int32_t pool,
                       int32_t k, float lam, int32_t flags, int32_t* items, float* scores,
                       float* mmr);
/* frecsys_mmr_select (above: the pool, the relevance, the cosine chain, the
 * greedy steps, the tie order and the outputs are stated there in full and
 * hold here to the bit) of caller-supplied pools against the context's ITEM
 * table: lists / list_scores are host [n][pool] from anywhere
 * (frecsys_rank_candidates, frecsys_similar, another retriever).  Per row
 * batch the pools are uploaded, div_gram_kernel forms G = T T^T over the
 * pool's item rows (v_mfma_f32_32x32x2_f32, one accumulator chain per element
 * over the padded dim: the chain above, pad columns add +0), and
 * div_select_kernel runs the greedy steps, one wave per row, reading row s_t
 * of G per step.  Workspace: frecsys_recommend's buffer and budget
 * (FRECSYS_RECOMMEND_WS_MB, read per call, changes no result bit); per row of a
 * batch 8 pool + 4 pool^2 + 12 k bytes, at least one row per batch; released
 * by frecsys_release_workspaces.  Rank-local: no collective.
 * FRECSYS_DIVERSIFY_VARIANT (read per call, changes no result bit): "gram" is
 * the pair above; "lazy" forms no Gramian -- the selection computes row s_t of
 * it per step from the item table (k pool d products instead of pool^2 d / 2,
 * no 4 pool^2 bytes, no "diversify.gram") -- and books 2 (k + 1) pool d + 5 k
 * pool flops and 4 (k + 1) pool d + 8 pool + 8 k bytes per row; unset: "gram",
 * the faster of the two at every shape measured.
 * FRECSYS_ERR_INVALID, before any device call: the common cases above, a null
 * context, a null pool array, an id >= items, a non-finite score in a filled
 * slot, a non-finite range (normalised mode).  Timer keys "diversify.gram"
 * and "diversify.select" (one launch each per Gramian sub-batch);
 * frecsys_work("diversify"): per row pool (pool + 1) d + 5 k pool flops, bytes
 * = 4 pool d + 4 pool^2 + 4 k pool + 8 pool + 8 k (12 k with mmr). */
int frecsys_diversify(frecsys_ctx* ctx, const int32_t* lists, const float* list_scores, int64_t n,
                      int32_t pool, int32_t k, float lam, int32_t flags, int32_t* items,
                      float* scores, float* mmr);
/* frecsys_recommend(side, rows, k = pool, flags & FRECSYS_REC_EXCLUDE_HISTORY,
 * item_mask) followed by frecsys_mmr_select (above: pool, relevance, cosine
 * chain, greedy steps, tie order and outputs as stated there, to the bit) on
 * the lists and scores it returns -- with the pools never leaving the device:
 * behind each row batch's scan the two kernels of frecsys_diversify run on the
 * batch's lists where the scan left them, and only the [rows][k] selection
 * goes to the host.  The slots beyond a row's eligible count are empty.  side
 * is USER or EVAL; flags is a subset of FRECSYS_REC_EXCLUDE_HISTORY |
 * FRECSYS_DIV_RAW_SCORES.  At lam = 1 items and scores are
 * frecsys_recommend(k)'s.  Workspace, knobs and rejections are
 * frecsys_recommend's, with 12 k more bytes per row of a batch, and the common
 * cases above; the Gramians lie behind the batch regions and are formed for
 * sub-batches of the batch's rows, 4 pool^2 bytes a row within a budget of the
 * same size (at least one row), so that a large pool does not shorten the
 * scan's batches: the workspace of this call is at most twice
 * FRECSYS_RECOMMEND_WS_MB plus one Gramian and the per-call regions, not once
 * as for frecsys_recommend.  FRECSYS_DIVERSIFY_VARIANT as in frecsys_diversify.
 * Unlike frecsys_diversify this call cannot look at the pools before the
 * device forms them: it assumes finite scores and a finite range.  A pool
 * whose range overflows has rel = 0, one with a non-finite score follows the
 * fp32 operations above as they come (frecsys_mmr_select rejects both).
 * Timer keys "recommend", "diversify.gram",
 * "diversify.select"; frecsys_work("recommend") as frecsys_recommend(k =
 * pool), frecsys_work("diversify") as frecsys_diversify. */
int frecsys_recommend_diverse(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                              int32_t k, int32_t pool, float lam, int32_t flags,
                              const uint8_t* item_mask, int32_t* items, float* scores, float* mmr);
/* Diversified lists by a determinantal point process (DPP): the greedy MAP
 * of Chen, Zhang and Zhou (NeurIPS 2018) over the same pools (no reference
 * counterpart).  Where MMR charges a candidate its largest cosine with a
 * selected item, the DPP charges it the part of it that lies in the span of
 * all of them: the selection greedily maximises det(L[sel, sel]), L =
 * diag(sqrt w) S diag(sqrt w), by an incremental Cholesky factorisation in
 * fp32.  The three calls below share one definition, fixed to the bit;
 * frecsys_dpp_select is that definition in scalar C++ on the host, and the two
 * device calls return its bits.
 *   Pool, relevance, similarity: frecsys_mmr_select's (above), to the bit: the
 * slots, p, rel_b (FRECSYS_DIV_RAW_SCORES or the min-max normalisation), the
 * chain g, n2_r, inv_r, and S(a, b) = (g * inv_a) * inv_b + 0.0f.
 *   Quality.  x_b = theta * rel_b, one fp32 multiply, then fminf(fmaxf(x_b,
 * -64.0f), 64.0f); w_b = dpp_exp2(x_b):  n = rintf(x) (to nearest, ties to
 * even), f = x - n (exact), q = c7, then q = fmaf(q, f, c_i) for i = 6 .. 0,
 * and the result is ldexpf(q, (int)n) (exact).  c_i = ln(2)^i / i! rounded to
 * fp32:  c0 = 0x1p+0, c1 = 0x1.62e430p-1, c2 = 0x1.ebfbe0p-3, c3 =
 * 0x1.c6b08ep-5, c4 = 0x1.3b2ab6p-7, c5 = 0x1.5d87fep-10, c6 = 0x1.430912p-13,
 * c7 = 0x1.ffcbfcp-17.  dpp_exp2 is a definition, not an approximation of
 * libm: host and device run this sequence.  It is within 1e-6 (relative) of
 * 2^x on [-64, 64]: the degree-7 remainder at |f| <= 1/2 is 5e-9, the eight
 * roundings add at most a few ulp.  theta = 0: w = 1 everywhere (pure
 * diversity); a larger theta moves the list toward the relevance order.
 *   Greedy selection.  State: r_b = n2_b > 0 ? 1.0f : 0.0f (the residual
 * variance; a zero item row starts at 0), a factor C with no rows, m = 0 DPP
 * steps.  For t = 0 .. min(k, p) - 1: E = the unselected filled slots with r_b
 * >= eps.
 *   E not empty (a DPP step): v_b = w_b * r_b + 0.0f for b in E; s_t is the
 * slot of E with the largest word score_key(v_b) << 32 | ~b (the largest v,
 * ties to the lower slot); gain[t] = v at s_t; delta = sqrtf(r at s_t); for
 * every unselected filled b other than s_t (inside E or not): acc =
 * fmaf(C[u][b], C[u][s_t], acc) over u = 0 .. m-1 ascending from +0, e =
 * (S(s_t, b) - acc) / delta, C[m][b] = e, r_b = fmaf(-e, e, r_b); then m += 1.
 *   E empty (the fallback): s_t is the lowest unselected filled slot, gain[t]
 * = 0.0f, and nothing else changes -- every later step is a fallback too.  In
 * a pool from frecsys_recommend that is score order.  rank(S) <= dim, so the
 * fallback starts after at most dim selections.
 *   Every multiply, subtraction, division and sqrt is one correctly rounded
 * fp32 operation, never contracted; an fma only where fmaf is written.
 *   Outputs (host), per row and t < k: items[t] = the id of s_t, scores[t] =
 * its pool score with its bits unchanged, and, unless gain is NULL, gain[t].
 * For t >= p: -1, -FLT_MAX and -FLT_MAX.
 * No output bit depends on the batch, the grid, the sub-batch, the workspace
 * budget, the item splits, the other rows, or where C is kept.
 * FRECSYS_ERR_INVALID for all three: pool outside [1, 1024], k outside
 * [1, pool], theta negative or not finite, eps outside (0, 1] or NaN, an
 * unknown flag bit, a negative row count, null outputs (items, scores) with
 * rows > 0.  Zero rows return FRECSYS_OK and touch nothing.
 *
 * frecsys_dpp_select: host only -- no context, no HIP call.  Arrays as for
 * frecsys_mmr_select, gain [n][k] or NULL.  Also FRECSYS_ERR_INVALID: a null
 * table or pool array, an id >= n_items, a non-finite score in a filled slot,
 * and (without FRECSYS_DIV_RAW_SCORES) a non-finite range. */
int frecsys_dpp_select(const float* item_table, int64_t n_items, int32_t dim, int64_t ld,
                       const int32_t* lists, const float* list_scores, int64_t n, int32_t pool,
                       int32_t k, float theta, float eps, int32_t flags, int32_t* items,
                       float* scores, float* gain);
/* frecsys_dpp_select (above, to the bit) of caller-supplied pools against the
 * context's ITEM table; batching as in frecsys_diversify.  Per sub-batch
 * div_gram_kernel forms the pool Gramians (frecsys_diversify's kernel,
 * unchanged) and dpp_select_kernel runs the greedy steps, one workgroup of 1, 2
 * or 4 waves per row (pool <= 256, <= 512, above).
 * The factor C ([k][pool] fp32 per row) lies in LDS when 4 k pool <= 40 KiB,
 * else in the workspace; FRECSYS_DPP_FACTOR=ws (read per call, changes no
 * result bit) keeps it in the workspace at every shape.  Workspace:
 * frecsys_recommend's buffer and budget; per row of a batch 8 pool + 4 pool^2
 * + 12 k bytes and, with C in the workspace, 4 k pool more; at least one row
 * per batch; released by frecsys_release_workspaces.  Rank-local.
 * FRECSYS_ERR_INVALID, before any device call: the common cases above, a null
 * context, a null pool array, an id >= items, a non-finite score in a filled
 * slot, a non-finite range (normalised mode).  Timer keys "diversify.gram"
 * (shared with the MMR calls) and "dpp.select" (one launch each per
 * sub-batch); frecsys_work("dpp"): per row pool (pool + 1) d + k (k - 1) pool
 * flops (the Gramian's triangle, then the factor's chains, sum over t < k of
 * 2 t pool, every step booked as a DPP step), bytes = 4 pool d + 4 pool^2 (the
 * item rows read, the Gramian written) + 4 k pool (its rows read) + 8 pool +
 * 4 k pool (the factor written) + 2 k (k - 1) pool (the factor read) + 8 k
 * (12 k with gain). */
int frecsys_diversify_dpp(frecsys_ctx* ctx, const int32_t* lists, const float* list_scores,
                          int64_t n, int32_t pool, int32_t k, float theta, float eps,
                          int32_t flags, int32_t* items, float* scores, float* gain);
/* frecsys_recommend(side, rows, k = pool, flags & FRECSYS_REC_EXCLUDE_HISTORY,
 * item_mask) followed by frecsys_dpp_select (above, to the bit) on the lists
 * and scores it returns, with the pools never leaving the device: behind each
 * row batch's scan the two kernels of frecsys_diversify_dpp run where the scan
 * left the lists, and only the [rows][k] selection goes to the host.  side is
 * USER or EVAL; flags is a subset of FRECSYS_REC_EXCLUDE_HISTORY |
 * FRECSYS_DIV_RAW_SCORES.  At eps = 1 step 0 takes the most relevant slot and
 * every residual that moved is below eps, so on a table without exactly
 * orthogonal pairs every later step is a fallback and the result is
 * frecsys_recommend(k)'s.  Workspace, knobs and rejections are
 * frecsys_recommend's, with 12 k more bytes per row of a batch, and the common
 * cases above; the Gramians and factors lie behind the batch regions in
 * sub-batches within a budget of the same size, as for
 * frecsys_recommend_diverse.  Like that call it cannot look at the pools
 * before the device forms them and assumes finite scores and a finite range.
 * Timer keys "recommend", "diversify.gram", "dpp.select";
 * frecsys_work("recommend") as frecsys_recommend(k = pool),
 * frecsys_work("dpp") as frecsys_diversify_dpp. */
int frecsys_recommend_dpp(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                          int32_t k, int32_t pool, float theta, float eps, int32_t flags,
                          const uint8_t* item_mask, int32_t* items, float* scores, float* gain);
/* ---- list quality: intra-list diversity, novelty, item exposure ----
 * What a serving configuration buys beside Recall / NDCG (no reference
 * counterpart): how varied each list is, how far down the popularity tail it
 * reaches, and how evenly the catalogue is exposed.  Four calls share the
 * definitions, which are stated here in full.
 *   Lists.  A row has list_k slots of item ids.  A negative id is an empty slot;
 * a repeated id is a slot of its own.  Cut-offs are k_list[q], 1 <= nk <= 32,
 * 1 <= k_list[q] <= min(1024, list_k), any order, repeats allowed.  For cut-off
 * K the filled slots are the non-negative ids among positions j < K: n of them,
 * in list order b = 0 .. n-1.
 *   ILD@K = 1 - the mean pairwise cosine of the filled slots by item factors,
 * all in float64: n2_b = sum_c y_bc^2 over the item row converted to double;
 * inv_b = n2_b > 0 ? 1 / sqrt(n2_b) : 0 (a zero row has cosine 0 with
 * everything, as for the MMR calls); yh_b = inv_b y_b; s_b = sum_{a<b} yh_a;
 * T_b = yh_b . s_b; C(K) = sum_{b<n} T_b; ild = n >= 2 ? (float)(1 - C /
 * (n (n - 1) / 2)) : 0.0f.  The running sum makes every cut-off one O(K d)
 * sweep; no K x K Gramian is formed.  The result is not clamped: a list of one
 * item repeated gives about +-1e-16, not exactly 0.
 *   Novelty@K = n >= 1 ? (float)(sum_{b<n} (double)item_weight[id_b] / n) :
 * 0.0f, with item_weight a host fp32 [n_items] array of the caller's (self
 * information -log2 of the item's popularity is the usual choice; the library
 * sums weights and takes no logarithm).  item_weight NULL: no novelty, and the
 * novelty output must be NULL too.
 *   Exposure.  exposure[q * n_items + i], int64: the filled slots with id i
 * among positions < k_list[q], summed over the rows of the call.  Integers, so
 * exact and independent of any order.
 *   Outputs.  ild, novelty: host [n * nk]; exposure: host [nk * n_items]; each
 * may be NULL, not all.
 *   What is bit-stable.  Exposure is exact integers, and the summary below is
 * one host function of them for every caller: device and host agree bit for
 * bit.  The device fixes the reduction order of ILD and
 * novelty by the padded dim and the list alone: a row's output bytes do not
 * depend on the batch, the item splits, the sub-batch, FRECSYS_RECOMMEND_WS_MB,
 * FRECSYS_RECOMMEND_SPLITS, the other rows or the order of the rows.  Device
 * against host ILD and novelty satisfy |a - b| <= 2^-23 max(1, |b|): every sum
 * is float64, reordering moves it by about (K + Dp) 2^-52, and what remains is
 * the final rounding to fp32 on each side, half an ulp each.
 *   FRECSYS_ERR_INVALID, before any device call and any write: k_list null or
 * nk outside [1, 32], a cut-off out of range, every output null, novelty
 * without item_weight or item_weight without novelty, a non-finite weight, a
 * negative row count, n * list_k beyond int64, an id >= n_items in any slot of
 * caller lists (the slots past the largest cut-off included).  Zero rows return
 * FRECSYS_OK and touch nothing but a given exposure array, which is zeroed.
 *
 * frecsys_list_quality: the definition in scalar C++ on the host -- no context,
 * no HIP call.  item_table is row-major [n_items][ld] with ld >= dim >= 1 (it
 * may be NULL when ild is); lists is [n][list_k]. */
int frecsys_list_quality(const float* item_table, int64_t n_items, int32_t dim, int64_t ld,
                         const int32_t* lists, int64_t n, int32_t list_k, const int32_t* k_list,
                         int32_t nk, const float* item_weight, float* ild, float* novelty,
                         int64_t* exposure);
/* The summary of one exposure row c[0 .. n_items) on the host.  M = the
 * eligible items (item_mask byte non-zero; NULL: all), S = sum of c_i over
 * them.  *coverage = (eligible i with c_i > 0) / M; *gini = sum_{i=1..M}
 * (2 i - M - 1) c_(i) / (M S) with c_(i) the eligible counts sorted ascending,
 * the numerator and M S accumulated exactly in 128-bit integers, each converted
 * to double (exact below 2^53; beyond it a rounding each, so the quotient is
 * then within 3 * 2^-53 relative of the exact ratio, not its rounding), then one
 * double division; both 0 when M == 0 or S == 0.  *total = S, *covered = the
 * count of covered items.  Every output may be NULL.  FRECSYS_ERR_INVALID: a
 * null array, n_items < 1, a negative count, a sum beyond int64. */
int frecsys_exposure_summary(const int64_t* exposure, int64_t n_items, const uint8_t* item_mask,
                             double* coverage, double* gini, int64_t* total, int64_t* covered);
/* frecsys_list_quality (above) of the lists a serving configuration produces,
 * without the lists leaving the device.  side, rows, flags and item_mask are
 * frecsys_recommend's.  pool == 0: the lists are frecsys_recommend(k = max
 * k_list)'s (lam is ignored, div_flags must be 0).  pool > 0: they are
 * frecsys_recommend_diverse(k = max k_list, pool, lam, div_flags)'s; div_flags
 * is 0 or FRECSYS_DIV_RAW_SCORES.  With a ground truth (gt_ptr / gt_items,
 * row i belongs to query row i; recall and ndcg then both given, host [n_rows *
 * nk]) Recall / NDCG of the same lists come back too, by frecsys_rank_metrics'
 * kernel: frecsys_list_metrics of those lists, bitwise.  Without one gt_ptr,
 * recall and ndcg are all NULL.  Per row batch: the scan, the two MMR kernels
 * (pool > 0), the metrics kernel (ground truth), then quality_kernel -- one wave
 * per row closes the filled slots up in LDS and sweeps them once with the next
 * four item rows in flight, lanes owning columns of the padded dim, one joint
 * butterfly for (y.y, y.s) per slot -- and exposure_kernel, 64-bit integer
 * atomics into [nk][n_items] counts that stay on the device across the batches
 * and are copied to the host once.  Workspace: frecsys_recommend's buffer and
 * budget (the MMR stage's as for frecsys_recommend_diverse) with 8 nk more bytes
 * per row of a batch, and outside that budget 4 nk + 4 n_items (weights) +
 * 8 nk n_items (counts) bytes; released by frecsys_release_workspaces.
 * FRECSYS_ERR_INVALID: the cases above, then pool outside [1, 1024], max k_list
 * above pool ("k must be in [1, pool]"), lam outside [0, 1] or NaN, an unknown
 * flag, recall / ndcg without a ground truth or the reverse, then
 * frecsys_recommend's and frecsys_rank_metrics' cases.  Timer keys "quality"
 * and "quality.exposure" (one launch each per row batch) beside "recommend",
 * "diversify.*" and "rank_metrics"; frecsys_work("quality"), every slot booked
 * as filled: per row 6 K d flops with ild (two dot products and an axpy per
 * slot), bytes = K (4 Dp + 4, + 4 with novelty) + 4 nk per output, + 8 K nk
 * for the exposure's adds. */
int frecsys_rank_quality(frecsys_ctx* ctx, int32_t side, const int64_t* rows, int64_t n_rows,
                         int32_t flags, const uint8_t* item_mask, const int32_t* k_list,
                         int32_t nk, int32_t pool, float lam, int32_t div_flags,
                         const float* item_weight, const int64_t* gt_ptr, const int32_t* gt_items,
                         float* ild, float* novelty, float* recall, float* ndcg,
                         int64_t* exposure);
/* The same two kernels on caller lists [n][list_k] (host) against the
 * context's ITEM table: the lists are uploaded in row batches within the
 * recommend budget (4 list_k + 8 nk bytes per row, at least one row), as
 * frecsys_diversify uploads its pools.  No ground truth here:
 * frecsys_list_metrics takes the same lists on the host.  FRECSYS_ERR_INVALID
 * also for a null context, list_k < 1, no item embeddings, null lists. */
int frecsys_lists_quality(frecsys_ctx* ctx, const int32_t* lists, int64_t n, int32_t list_k,
                          const int32_t* k_list, int32_t nk, const float* item_weight, float* ild,
                          float* novelty, int64_t* exposure);
/* Train-loss diagnostics (ComputeLosses / PrintLosses, ials.h:226-305,
 * safer2.h:337-413), all rows of both sides on every rank: observed = sum
 * over every USER-side interaction of (v.u - 1)^2 (per-user fp32 sums,
 * total in double), unobserved = sum_ij (U^T U)_ij (V^T V)_ij (unweighted
 * Gramians, double), and the squared row norms of U and V (host [n_users]
 * and [n_items]).  Any output pointer may be NULL.  The Gramian slots used
 * by the solves are left untouched. */
int frecsys_train_stats(frecsys_ctx* ctx, double* observed, double* unobserved,
                        float* user_norm2, float* item_norm2);
/* Sum over every row of `side` of ||X_r - snapshot_r||^2 (double), against
 * the snapshot frecsys_snapshot took: the residual norms of
 * --print_residual_stats, squared (StepU's sum of squared row changes,
 * safer2.h:475-478 / erm_mf.h:434-437; StepV's (V - V_prev).norm(),
 * safer2.h:550-553 / erm_mf.h:508-511 / cvar_mf.h:533-536). */
int frecsys_snapshot_residual(frecsys_ctx* ctx, int32_t side, double* sq);
/* Cumulative event counters of the context (never reset):
 *   "hspace_reruns"   solves of a side rerun on the d-space path after a
 *                     history-space pivot failure (a silent slow path);
 *   "tagged_timeouts" device polls of the tagged-word exchange of the
 *                     tridiagonalisation that timed out (each one poisons
 *                     the basis and forces a rerun);
 *   "ws_shrinks"      wide workspaces (d = 257..1024) cut below their
 *                     budget by a failed device allocation: a halved batch,
 *                     fewer long-history slabs, or the register-staged SYRK
 *                     instead of the pre-split table -- results unchanged;
 *   "cg_iterations"   sum of the CG iteration counts of every entity solved
 *                     by frecsys_solve_side_cg;
 *   "cg_unconverged"  entities whose CG stopped at max_iterations;
 *   "two_stage_certified", "two_stage_fallback_rows"  rows of
 *                     frecsys_recommend_two_stage that stage 2 certified, and
 *                     rows it re-ran through the exact scan.
 * And two values that are no sums: "recommend_splits", the item splits the
 * last frecsys_recommend call ran with; "live_device_bytes", the device
 * memory every context of the process holds now in buffers of its own
 * (process-wide, so what a destroyed context gave back can be read through
 * any other: it returns to its earlier value when nothing leaked).
 * No reference counterpart (diagnostics of the MI355X path). */
int frecsys_counter(frecsys_ctx* ctx, const char* what, int64_t* value);
/* Block until all queued device work is done (all calls already do). */
int frecsys_synchronize(frecsys_ctx* ctx);
/* Free the wide-dim workspaces (batch workspace of A tiles, long-history
 * slabs, pre-split table, history-space wide bucket); the next solve sizes
 * them again within FRECSYS_WIDE_WS_MB and a quarter of the then free device
 * memory each.  The ranking workspace of frecsys_recommend and its
 * relatives (the list ids of frecsys_sampled_metrics among them) and the
 * inverse norms of frecsys_similar go too; the next such
 * call sizes them again. For a caller that needs the device memory between phases
 * (evaluation, another model).  No reference counterpart: the reference's
 * per-thread Eigen temporaries are freed per entity. */
int frecsys_release_workspaces(frecsys_ctx* ctx);

/* ---- profiling hooks (bench.py) ----
 * Kernel time accumulated with HIP events recorded on the library's
 * streams around each launch of kernel class `what` ("solve_user",
 * "solve_item", "solve_eval", "gramian", "user_loss", "allgather",
 * "allreduce"; per solve also "<solve>.dspace" (d x d solve of the long
 * histories), "<solve>.split" (partial SYRKs of the longest of them),
 * "<solve>.basis" (tridiagonalisation of G + rotation of the other side),
 * "<solve>.hspace" (history-space solve), "<solve>.rotate", "<solve>.cg"
 * (the conjugate-gradient kernel of frecsys_solve_side_cg))
 * since the last frecsys_timing_reset. */
int frecsys_timing(const frecsys_ctx* ctx, const char* what, double* total_ms,
                   int64_t* launches);
int frecsys_timing_reset(frecsys_ctx* ctx);
/* The algorithmic work the library launched under timer key `what` since
 * the last frecsys_timing_reset (SURVEY 8(d) definitions at the logical
 * dim d, per entity of h assembly rows): "<solve>.dspace" h d (d+1) +
 * d^3/3 + 2 d^2 flops (the SYRK of split entities is "<solve>.split"'s),
 * gather bytes h d 4 + h 4 + 8 + d 4; "<solve>.hspace" h^2 d + h^3/3 +
 * 4 h d flops, bytes 2 h d 4 + h 4 + 8 + 4 d 4; "gramian" 2 N d^2 flops over
 * the rows this rank formed, N d 4 bytes; "user_loss" 2 nnz d + 2 N d^2
 * flops, nnz d 4 + nnz 4 + (N+1) 8 + N 4 bytes.  `launches` counts the
 * timed calls, as frecsys_timing does.  Any output may be NULL. */
int frecsys_work(const frecsys_ctx* ctx, const char* what, double* flops, double* bytes,
                 int64_t* entities, int64_t* launches);
/* The context's default threshold: the longest assembly history (h_eff) the
 * history-space path takes on a side that has no threshold of its own (0: that
 * path is off); longer histories run the d-space solve.  A side can differ
 * (Dp = 512: users 320 beside this 256), so to tell which rows a solve puts in
 * which space, ask frecsys_history_space_max_h_side() for the solved side. */
int32_t frecsys_history_space_max_h(const frecsys_ctx* ctx);
/* The same for one solved side (FRECSYS_SIDE_USER / _ITEM: the rows solved by
 * frecsys_solve_side(side)); the sides differ where a default or
 * FRECSYS_DUAL_MAX_H_USER / _ITEM sets them apart (Dp = 512: users 320,
 * items 256).  0 for another side or with the path off. */
int32_t frecsys_history_space_max_h_side(const frecsys_ctx* ctx, int32_t side);

/* ---- diagnostics (tests) ----
 * The basis the history-space solve uses for G[side]: G = Q T Q^T with Q
 * orthogonal (Dp x Dp, row-major) and T tridiagonal (diag[Dp],
 * sub[Dp]: T(k+1, k), sub[Dp-1] = 0); Dp = frecsys_padded_dim(dim).  No
 * reference counterpart. */
int frecsys_debug_basis(frecsys_ctx* ctx, int32_t side, float* q, float* diag, float* sub);
/* The two diagonal-block factorisations of the blocked Cholesky (the
 * 32x32 pivot blocks of every solve): for each of n_tiles row-major 32x32
 * SPD tiles a[t], linv[t] = L^-1 with L L^T = a[t] (lower; upper part 0),
 * by the MFMA-blocked factor (blocked != 0) or the lane recurrence;
 * ok[t] = 0 on a non-positive pivot.  No reference counterpart (Eigen's
 * LLT inner kernel, ials.h:140). */
int frecsys_debug_diag_factor(frecsys_ctx* ctx, int32_t blocked, int32_t n_tiles, const float* a,
                              float* linv, int32_t* ok);

#ifdef __cplusplus
}
#endif
#endif /* FRECSYS_HIP_H_ */
