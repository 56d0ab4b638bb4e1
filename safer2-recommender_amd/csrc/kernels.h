// kernels.h -- launch interface between the C-ABI host code (capi.hip, train.hip,
// serve.hip) and the gfx950 kernels (solve.hip, gramian.hip, loss.hip).  Internal header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

namespace frecsys_hip {

// One entry of the solve queue: entity row, its history length and the
// offset of its history in the CSR column array (16 B, one load).
struct QueueRec {
  int32_t entity;
  int32_t h;
  int64_t p0;
};

// One partial SYRK of a long history: queue position, virtual history
// positions [k0, k1), output slab.
struct SplitWork {
  int32_t pos;
  int32_t k0;
  int32_t k1;
  int32_t slab;
};

// Everything one launch of the per-entity solve needs (device pointers).
struct SolveArgs {
  int kind;                 // FRECSYS_KIND_*
  int quirk;                // reproduce the ProjectV tail double-count
  const int64_t* row_ptr;   // CSR of the solved side
  const int32_t* col;
  int64_t row_lo;           // first entity of this launch (small kernel)
  int64_t n_rows;           // entities in this launch
  const QueueRec* order;    // [n_rows] longest history first (tiled kernel)
  unsigned int* counter;    // work-queue head, zeroed by the launcher
  const float* X;           // other side's embeddings, ld = Dp
  int64_t n_other;          // rows of the other side (for lambda)
  const float* G;           // Dp x Dp Gramian of the other side
  const float* E;           // current embeddings of the solved side (CVaR)
  float* out;               // solved side's embeddings, ld = Dp
  float reg, reg_exp, w, alpha, eta;
  int lambda_is_reg;           // lambda = reg for every entity
  const float* entity_weight;  // [rows of side] omega, or nullptr (-> 1)
  const float* entity_reg;     // [rows of side] item_reg_
  const float* other_weight;   // [rows of other side] nu
  unsigned long long* fail;    // atomicMin(entity + 1) on a non-SPD pivot
  int debug_skip;              // diagnostic ablation mask (0 in production)
  int chol_sched;              // the dataflow Cholesky's static worker schedule (chol_sched.h): 1 on
  unsigned long long* prof;    // diagnostics: per-phase cycle sums [16] (nullptr = off)
  // long-history split (tiled and wide kernels; nullptr / 0 = none)
  const int2* split;           // [n_split] per queue position: first slab, slab count
  int64_t n_split;
  float* slabs;                // [slabs][split_slab_floats(Dp)]
  const SplitWork* work;       // [n_work] partial SYRK items
  int64_t n_work;
  // wide dims: the pre-split copy of X (wide.h wide_xsplit_*), or nullptr
  const char* xsplit;
};

// Partition-independent Gramian.  The rows of a side are cut
// into fixed leaves (rows per leaf from the side's row count alone) and the
// leaves into ngroup = min(kGramGroups, leaves) runs of consecutive leaves.
// A leaf's partial is one workgroup's fixed-order accumulation, a group's
// slab the sum of its leaves in leaf order, and G the sum of the group slabs
// in group order: the same additions whichever rank computes which group, so
// G is bitwise the same at every world size (ranks own whole groups and
// exchange group slabs, never partially reduced sums).
constexpr int kGramGroups = 16;
struct GramPlan {
  int64_t n = 0;        // rows of the side
  int64_t rpl = 0;      // rows per leaf
  int64_t nleaf = 0;
  int ngroup = 0;
  size_t slab_floats = 0;  // floats of one leaf / group slab (lower tiles, or Dp^2 at Dp <= 16)
};
GramPlan gram_plan(int Dp, int64_t n);
inline int64_t gram_group_leaf(const GramPlan& p, int g) {
  return p.ngroup ? (int64_t)g * p.nleaf / p.ngroup : 0;
}
// Groups [lo, hi) of rank `rank` of `world` (contiguous, balanced by count).
inline void gram_owned_groups(const GramPlan& p, int world, int rank, int* lo, int* hi) {
  *lo = (int)((int64_t)p.ngroup * rank / world);
  *hi = (int)((int64_t)p.ngroup * (rank + 1) / world);
}
// Leaf-workspace floats for computing groups [g_lo, g_hi).
size_t gram_leaf_floats(const GramPlan& p, int g_lo, int g_hi);

struct GramArgs {
  const float* X;        // ld = Dp
  const float* w;        // per-row weight (absolute row index) or nullptr
  float* partials;       // leaf workspace (gram_leaf_floats)
  float* gslabs;         // [plan.ngroup][plan.slab_floats] group slabs
  GramPlan plan;
  int g_lo, g_hi;        // groups this launch computes
  // set by the launcher: rows [row0, row0 + n) = the leaves of the groups
  int64_t row0;
  int64_t n;
};

struct LossArgs {
  const int64_t* row_ptr;
  const int32_t* col;
  int64_t row_lo, n_rows;
  const float* U;        // ld = Dp (rows of the side)
  const float* V;        // items, ld = Dp
  const float* G;        // Dp x Dp
  float beta;
  int half;
  float* out;            // [rows of side]
  float* quad;           // [rows of side] scratch: u^T G u (Dp >= 32); with quad_parts > 0
                         // [quad_parts][n_rows] partial sums by launch row (rotate_quad)
  int quad_parts;
  void* gsplit;          // Dp = 512 / 1024: scratch for G's split image (basis_split_bytes)
  int raw;               // 1: out[e] = sum_j (x_j . u - 1)^2 only (train stats)
  hipEvent_t ev_gather;  // recorded right before the gather kernel (timing), or nullptr
};


// History-space ("dual") solve of the short-history entities (dual.hip).
// With G = Q T Q^T (Q orthogonal, T tridiagonal) and M = mu*G + lam*I,
// A = M + Xt^T Xt, b = Xt^T s  (Xt = the history rows scaled by sqrt of
// their A-weight, s = the matching rhs coefficients) is solved as
//   x = Q (mu*T + lam*I)^-1 Y^T z,  z = (I + Y (mu*T + lam*I)^-1 Y^T)^-1 s,
// Y = Xt Q (push-through identity): an h x h SPD system instead of d x d.
struct DualArgs {
  int kind;                 // FRECSYS_KIND_IALS / WEIGHTED_U / WEIGHTED_V
  int quirk;
  int Dp;
  const QueueRec* order;    // [n_rows] this launch's entities
  int64_t n_rows;
  const int32_t* col;       // CSR columns of the solved side
  const float* Xrot;        // other side rotated into the T basis: X Q, ld Dp
  const float* tdiag;       // [Dp] diagonal of T
  const float* toff;        // [Dp] T(k+1, k)
  // Cholesky basis (launch_chol_basis: one M for every entity, Xrot = X L^-T):
  // the LDL table is the unit one and *basis_status = 0 fails the launch
  int unit_m;
  const float* basis_status;
  int64_t n_other;
  // position-blocked buffers (64 positions per block, k-major inside a
  // block: every access by consecutive positions is coalesced), position =
  // pos0 + index in this launch's order slice:
  //   out_rot[blk][k][64]     Y^T (c.*z), then x'
  //   table[blk][3][Dp][64]   l_k, D^-1/2, D^-1 of mu*T + lam*I
  float* out_rot;
  float* table;
  int64_t pos0;
  float reg, reg_exp, w, alpha;
  int lambda_is_reg;
  const float* entity_weight;
  const float* entity_reg;
  const float* other_weight;
  unsigned long long* fail;
  int debug_skip;  // ablation only: 1 SYRK, 2/4/8/16 Cholesky parts, 64 Y^T z, 128 recurrence
  int chol_sched;  // the dataflow Cholesky's static worker schedule (chol_sched.h): 1 on
  unsigned long long* prof;  // diagnostics: per-phase cycle sums [16] (nullptr = off)
};

// Largest history-space tile count built (h_eff <= 32 * kDualMaxTiles).
constexpr int kDualMaxTiles = 8;

// Conjugate-gradient solve (cg.hip; Dp <= 256): workgroup b takes the queue
// entities order[bstart[b] .. bstart[b + 1]), at most kCgE; history rows in
// chunks of kCgU passes of 64 / GP rows (GP = the power of two >= Dp / 4
// lanes per row).
constexpr int kCgE = 16;
constexpr int kCgU = 8;
// An entity of more than kCgCoopRows (virtual) history rows is streamed by
// all four waves of its workgroup; a batch holds as many entities (<= kCgE)
// as fit kCgBatchRows history rows, at least one (cg_plan_batches).
constexpr int kCgCoopRows = 256;
constexpr int kCgBatchRows = 4096;
struct CgArgs {
  int kind;                 // FRECSYS_KIND_IALS / WEIGHTED_U / WEIGHTED_V
  int quirk;                // WEIGHTED_V: the ProjectV tail double-count
  int Dp, dim;
  const QueueRec* order;    // LPT queue of the solved side
  const int32_t* bstart;    // [n_batches + 1] queue position of every batch's first entity
  int64_t n_batches;
  const int32_t* col;       // CSR columns of the solved side
  const float* X;           // other side's embeddings, ld = Dp
  int64_t n_other;
  const float* G;           // Dp x Dp Gramian of the other side
  float* out;               // solved side's embeddings, ld = Dp
  float reg, reg_exp, w, alpha;
  int lambda_is_reg;
  const float* entity_weight;
  const float* entity_reg;
  const float* other_weight;
  int max_iter;
  float tol;
  int32_t* iters;             // [rows of side]: i of every solved entity
  unsigned long long* stats;  // [2]: += sum of i, += entities stopped at the cap
  unsigned long long* fail;   // atomicMin(entity + 1) on a non-finite result row
};
size_t cg_lds_bytes(int Dp);
// Host: the batches of the queue order[0..n) (consecutive entities).
void cg_plan_batches(const QueueRec* order, int64_t n, std::vector<int32_t>* bstart);
hipError_t launch_cg(const CgArgs& a, hipStream_t s);

// Explanations (explain.hip; Dp <= 256): per query row the d x d system of
// frecsys_solve_side (kinds IALS / WEIGHTED_U) assembled and factored once,
// W = A^-1 V_targets^T by substitution in groups of kExplainGroup targets,
// and contrib[j][t] = c_j (y_j . w_t) for every history entry j.  Query row i
// of the batch is row qrows[r0 + i] (or r0 + i) of the side's CSR; its
// targets are tgt[tgt_ptr[r0 + i] - tgt_base .. tgt_ptr[r0 + i + 1] - tgt_base).
// Pair p of the batch (the targets of its rows in order) has its h
// contributions, in CSR order, at contrib[coff[i] + t h ..), t its index
// among the row's targets.  launch_explain fills contrib; launch_explain_select
// reads it: score[p] (the sum of the pair's contributions), and the `top`
// largest by (contribution descending, CSR position ascending) with their
// history item ids, -1 / 0 behind them.
constexpr int kExplainGroup = 32;   // right-hand sides of one substitution
constexpr int kExplainChunk = 256;  // history rows one sweep of the second pass takes (8 waves x 32)
constexpr int kExplainMaxTop = 32;
struct ExplainArgs {
  int kind;                  // FRECSYS_KIND_IALS / WEIGHTED_U
  int Dp;
  const int64_t* row_ptr;    // CSR of the explained side
  const int32_t* col;
  const int64_t* qrows;      // CSR row of every query row of the call, or nullptr
  int64_t r0, n;             // this batch: query rows r0 .. r0 + n - 1
  const int64_t* tgt_ptr;    // [rows of the call + 1]
  const int32_t* tgt;        // the batch's target ids, each in [0, n_other)
  int64_t tgt_base;          // tgt_ptr[r0]
  const int64_t* coff;       // [n] first contribution of every row of the batch
  const int32_t* prow;       // [pairs of the batch] row of the batch (select)
  const int32_t* order;      // [n] the rows of the batch, most work first (a permutation)
  const float* X;            // items, ld = Dp
  int64_t n_other;
  const float* G;            // Dp x Dp Gramian of the items
  float reg, reg_exp, w;
  int lambda_is_reg;
  const float* entity_weight;  // [rows of side] omega, or nullptr (-> 1)
  float* wws;                // [workgroups][kExplainGroup][explain_ld(Dp)]: W of the group in flight
  float* contrib;            // the batch's contributions
  unsigned long long* fail;  // atomicMin(entity + 1) on a non-SPD pivot
  int top;                   // 1 .. kExplainMaxTop
  float* score;              // [pairs of the batch]
  int32_t* top_items;        // [pairs][top]
  float* top_contrib;        // [pairs][top]
};
int explain_ld(int Dp);       // floats per row of a W slot: Dp rounded up to whole tiles
size_t explain_lds_bytes(int Dp);
// `grid` workgroups, each with its own W slot, take the rows grid apart.
hipError_t launch_explain(const ExplainArgs& a, int grid, hipStream_t s);
hipError_t launch_explain_select(const ExplainArgs& a, int64_t n_pairs, hipStream_t s);

hipError_t launch_solve(int Dp, const SolveArgs& a, hipStream_t s);
// Diagnostics: n 32x32 tiles (row-major) -> L^-1 of each (blk: the
// MFMA-blocked diagonal factor, else the lane recurrence), ok[n].
hipError_t launch_debug_diag(const float* A, float* Linv, int* ok, int n, int blk, hipStream_t s);
// Partial SYRKs of the split entities (a.work[0..n_work)) into a.slabs.
hipError_t launch_split_syrk(int Dp, const SolveArgs& a, hipStream_t s);
size_t split_slab_floats(int Dp);
// LDL^T of every entity's tridiagonal mu*T + lam*I (one thread per entity,
// a.order[0..n_rows)) into a.table.
hipError_t launch_dual_ldl(const DualArgs& a, hipStream_t s);
// out_rot rows of a.order[0..n_rows): v -> L^-T D^-1 L^-1 v (one thread per
// entity, table rows as written by launch_dual_ldl).
hipError_t launch_dual_sweep(const DualArgs& a, hipStream_t s);
// One launch per history bucket: every entity of a.order has
// 32*(tiles-1) < h_eff <= 32*tiles.
hipError_t launch_dual(int tiles, const DualArgs& a, hipStream_t s);
// The wide bucket (dual.hip): 256 < h_eff <= 512 at Dp = 512 / 1024, the
// entities a.order[0..n_rows) (positions a.pos0..) through HBM workspaces:
// zs (dual_wide_zs_bytes per entity), slots (dual_wide_slot_floats per
// entity), zbuf (512 floats per entity); Cholesky failures into fail.
constexpr int kDualWideMaxH = 512;
size_t dual_wide_zs_bytes(int Dp);
size_t dual_wide_slot_floats();
hipError_t launch_dual_wide(const DualArgs& a, void* zs, float* slots, float* zbuf,
                            unsigned long long* fail, hipStream_t s);
// wide_chol_kernel<16> over n Cholesky slots (row-major 32 x 32 tiles of a
// 512 x 512 SPD matrix + its rhs): solution of slot i into out[512 i ..),
// a failure reported as order[i].entity; only the tiles holding the
// h_eff = order[i].h (+ the tail quirk's rows when quirk_v) rows are factored.
hipError_t launch_wide_chol_slots(const QueueRec* order, int64_t n, float* slots, float* out,
                                  unsigned long long* fail, int quirk_v, hipStream_t s);
// Householder tridiagonalisation G = Q T Q^T of a Dp x Dp symmetric matrix
// (one workgroup): T's diagonal / subdiagonal, the reflectors (row k of Vh,
// entries k+1..Dp-1) and their tau.  With Q (only when tridiag_forms_q(Dp)):
// Q itself too, row-major, formed by workgroups of the same launch as the
// reflectors are published (work: tridiag_work_floats(Dp)), and with
// img_q / img_qt the split images of Q and Q^T (launch_split_basis's layout).
hipError_t launch_tridiag(const float* G, int Dp, float* tdiag, float* toff, float* Vh,
                          float* tau, hipStream_t s, float* work = nullptr, float* Q = nullptr,
                          void* img_q = nullptr, void* img_qt = nullptr,
                          unsigned* tcount = nullptr);
bool tridiag_forms_q(int Dp);
size_t tridiag_work_floats(int Dp);
// Q = H_0 H_1 ... H_{Dp-3} from the reflectors, row-major Dp x Dp; with
// img_q / img_qt also the split images of Q and Q^T (launch_split_basis's
// layout, basis_split_bytes each; Dp a multiple of 32).
hipError_t launch_form_q(const float* Vh, const float* tau, int Dp, float* Q, hipStream_t s,
                         void* img_q = nullptr, void* img_qt = nullptr);
// The split image of B = (trans ? Q^T : Q) for launch_rotate: Dp * Dp * 3
// bf16 (16-B granules in MFMA fragment order).
size_t basis_split_bytes(int Dp);
hipError_t launch_split_basis(const float* Q, int Dp, int trans, void* out, hipStream_t s);
// Cholesky basis of M = mu*G + lam*I (one workgroup): XT = L^-T (Dp x Dp,
// row-major, upper triangular) with M = L L^T; status[0] = 1, or 0 on a
// non-positive pivot.  work: chol_basis_work_floats(Dp).  Dp = 64..256, 512,
// 1024 (T = 32: 7 staging tiles beside the 31-tile panel in the 160 KB of
// LDS, spectral.hip chol_basis_stage_tiles).
size_t chol_basis_work_floats(int Dp);
hipError_t launch_chol_basis(const float* G, int Dp, float mu, float lam, float* work, float* XT,
                             float* status, hipStream_t s);
// Y[row] = X[row] * B with B given by its split image (launch_split_basis),
// fp32-accurate products on the bf16 matrix cores,
// for rows r0..r0+n-1, or for the entities rows[0..n) when rows != nullptr
// (Y: ld Dp; X: ld Dp, or with x_blocked the position-blocked layout of
// DualArgs::out_rot, X row r = position r).  Dp = 64 .. 256, 512, 1024.
// Rows of the other side that a side's history-space entities read (the
// forward rotation's subset): mark[col[p]] = 1 over their histories.
hipError_t launch_mark_rows(const QueueRec* order, int64_t n, const int32_t* col, uint8_t* mark,
                            hipStream_t s);
hipError_t launch_rotate(const float* X, const QueueRec* rows, int64_t r0, int64_t n,
                         const void* bsplit, float* Y, int Dp, hipStream_t s, int x_blocked = 0);
// Dp = 512 / 1024: qpart[b * n + r] = sum over the columns of 128-block b of
// (X B)[r] .* X[r] for rows r0 .. r0+n-1 (u^T G u partials, B = G).
hipError_t launch_rotate_quad(const float* X, int64_t r0, int64_t n, const void* bsplit,
                              float* qpart, int Dp, hipStream_t s);
// Column blocks (partial sums per row) launch_rotate_quad writes at Dp.
int rotate_quad_parts(int Dp);

__host__ __device__ inline int64_t blk_v(int64_t p, int k, int Dp) {
  return ((p >> 6) * Dp + k) * 64 + (p & 63);
}
__host__ __device__ inline int64_t blk_t(int64_t p, int j, int k, int Dp) {
  return ((p >> 6) * 3 * Dp + j * Dp + k) * 64 + (p & 63);
}
// The leaves of groups [a.g_lo, a.g_hi) into a.partials, each group summed
// into its slab a.gslabs[g].
hipError_t launch_gramian(int Dp, const GramArgs& a, hipStream_t s);
// G = sum of the plan's group slabs in group order, mirrored (Dp x Dp).
hipError_t launch_gram_final(int Dp, const GramPlan& p, const float* gslabs, float* G,
                             hipStream_t s);

// iALS++ block step (pp.hip; ialspp.h:85-145, 351-424).
struct PPArgs {
  const QueueRec* order;    // entities of the launch (LPT order)
  int64_t n_rows;
  const int32_t* col;       // CSR columns of the solved side
  const int32_t* rix;       // rating index per CSR entry (nullptr: the CSR position)
  float* pred;              // prediction vector, by rating index
  const float* X;           // other side, ld Dp
  const float* G;           // Gramian of the other side, Dp x Dp
  float* E;                 // solved side, ld Dp (block updated in place)
  int Dp, start, bw;        // block columns [start, start + bw), bw <= 128
  int kind;                 // KIND_IALS (iALS++), KIND_WEIGHTED_U / _V (SAFER2++)
  float reg, reg_exp, w, alpha;
  const float* entity_weight;  // U: omega (nullptr -> 1)
  const float* entity_reg;     // V: item_reg_
  const float* other_weight;   // V: nu_u = omega_u / |H_u|
  int64_t n_other;
  float* resid;             // [n_rows] squared delta norms, or nullptr
  unsigned long long* fail;
};
// Sharded block step: the prediction updates of rows [0, n) outside [lo, hi)
// replayed from old ([n][bw], the block before the step) and a.E (after).
hipError_t launch_pp_refresh(const PPArgs& a, const int64_t* row_ptr, const float* old,
                             int64_t n, int64_t lo, int64_t hi, hipStream_t s);
hipError_t launch_pp_step(const PPArgs& a, hipStream_t s);
// PredictDataset over the CSR rows 0..n_rows-1 (E = the rows' embeddings).
hipError_t launch_pp_predict(const PPArgs& a, const int64_t* row_ptr, int64_t n_rows,
                             hipStream_t s);

// Fold-in scoring + top-k (topk.hip): rows r0..r0+n-1 of X against the m
// rows of Y; S: [n][m] workspace; out: [n][k].
hipError_t launch_eval_topk(const float* X, int64_t r0, int64_t n, const float* Y, int64_t m,
                            int Dp, const int64_t* row_ptr, const int32_t* col, int k, float* S,
                            int32_t* out, hipStream_t s);

// Fused scoring + streaming top-K (recommend.hip): the k best eligible items
// of each of n query rows, with their scores, without a rows x items score
// buffer.  Query row i of the batch is row qrows[r0 + i] (or r0 + i when
// qrows == nullptr) of X; an item j is eligible when bit j of maskw is set
// (the caller folds the item mask and j < m into it) and, with row_ptr / col /
// bitmap given, j is not in that row's CSR history.
struct RecommendArgs {
  const float* X;            // query table, ld = Dp
  const int64_t* qrows;      // table row of every query row of the call, or nullptr
  int64_t r0, n;             // this batch: query rows r0 .. r0 + n - 1
  const float* Y;            // items, ld = Dp
  int64_t m;                 // items
  int Dp;
  int k;                     // 1 .. 1024
  int splits;                // item splits, 1 .. recommend_max_splits(k, m)
  const int64_t* row_ptr;    // CSR of the query table's side, or nullptr (no exclusion)
  const int32_t* col;
  const uint32_t* maskw;     // [recommend_words(m)] eligibility bits of the items
  uint32_t* bitmap;          // [n][recommend_words(m)] history bits (workspace), or nullptr
  unsigned long long* cand;  // [n][splits][recommend_cap(k)] candidates (workspace)
  int32_t* counts;           // [n][splits] candidates kept per split (workspace)
  int32_t* out_items;        // [n][k]
  float* out_scores;         // [n][k]
  // frecsys_similar (X == Y): either one selects the scan's second instantiation
  const float* inv;          // [m] inverse row norms of Y: the score is the cosine; or nullptr
  int skip_self;             // != 0: query row i never lists id qrows[r0 + i]
};
// Candidate slots per (row, split): 4 k rounded up to a power of two, from
// 512 to 2048 (2 k at k = 1024: a 128-item tile always fits behind k kept
// candidates; the room beyond k is what spaces the compactions).
int recommend_cap(int k);
// 32-bit words per row of the eligibility bitmaps: 4 per 128-item tile.
int64_t recommend_words(int64_t m);
// Largest split count: one 128-item tile per split at least, and splits * k
// candidates within the merge kernel's LDS.
int recommend_max_splits(int k, int64_t m);
hipError_t launch_recommend(const RecommendArgs& a, hipStream_t s);
// The history bitmaps of a row batch alone, as launch_recommend fills them
// (rec_history_kernel): bitmap[n][recommend_words(m)] zeroed, then bit j of
// row i set for every j of the CSR history of query row r0 + i.
hipError_t launch_history_bits(const int64_t* row_ptr, const int32_t* col, const int64_t* qrows,
                               int64_t r0, int64_t n, int64_t m, uint32_t* bitmap, hipStream_t s);

// rec_merge_kernel alone: the k best of each row's a.splits lists, a.counts
// words each at a.cand + (row * a.splits + s) * cap, every list sorted
// descending; a.splits * a.k words within the merge kernel's LDS.  Reads
// a.n, a.k, a.splits, a.cand, a.counts, a.out_items, a.out_scores only.
hipError_t launch_recommend_merge(const RecommendArgs& a, int64_t cap, hipStream_t s);

// Two-stage recommend (twostage.hip; the definitions are
// frecsys_recommend_two_stage's in include/frecsys_hip.h).
//
// bf16 of an fp32 bit pattern by round-to-nearest-even, as its 16 bits; a NaN
// stays a NaN (quiet, its upper payload kept).  The host's frecsys_bf16_round
// and every device conversion are this one function.
__host__ __device__ inline uint32_t bf16_round_bits(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// 0 < |v| < 2^-126 for the bf16 pattern h: outside the certificate's proof.
__host__ __device__ inline bool bf16_subnormal(uint32_t h) {
  return (h & 0x7f80u) == 0u && (h & 0x7fu) != 0u;
}
// c(Dp) of the certificate's bound B = c(Dp) ||x|| max ||y||.
__host__ __device__ inline double two_stage_c(int Dp) {
  return 0x1p-7 + 0x1p-16 + 3.0 * (double)Dp * 0x1p-23;
}
// Width of the bf16 images: the MFMA's K is 16.
inline int two_stage_dh(int Dp) { return Dp < 16 ? 16 : Dp; }
// The item image: per 128-item tile and 16-B granule (8 consecutive columns)
// the tile's 128 items side by side -- image[(tile * Dh / 8 + g) * 128 + j] --
// so that a k-slab of a tile is one contiguous run, copied into LDS as it
// lies and read there as MFMA fragments.  Pad columns and the rows beyond m
// are zero.
size_t two_stage_image_bytes(int64_t m, int Dp);
// ts_convert_kernel: the image of the m rows of T, norms[r] = ||T[r]|| (the
// squares accumulated and the root taken in double), stats[0] = the bits of
// the largest norm (a NaN norm counts as the largest), stats[1] = the values
// whose bf16 is subnormal.
hipError_t launch_two_stage_convert(const float* T, int64_t m, int Dp, void* image, double* norms,
                                    unsigned long long* stats, hipStream_t s);
// ts_scan_kernel in rec_scan_kernel's place: RecommendArgs as for
// launch_recommend (a.k the pool), a.Y unused -- the items are read from
// `image`.  The score of (row, item) is the fp32 accumulator of
// v_mfma_f32_32x32x16_bf16 over the bf16 of both rows from +0, the k-steps in
// ascending order: the same in every tile, split, batch and grid.
hipError_t launch_two_stage_scan(const RecommendArgs& a, const void* image, hipStream_t s);
// ts_select_kernel: row i of the batch re-scores the filled slots of its pool
// (pool_items[i * pool ..), -1 beyond the fill; ids distinct) by the chain
// acc = fmaf(y[c], x[c], acc), c ascending from +0 -- recommend.hip's score,
// bit for bit -- and lists the k best by (score descending, id ascending),
// -1 / -FLT_MAX beyond the fill; certified[i] as the header defines it.
struct TwoStageSelectArgs {
  const float* X;            // query table, ld = Dp
  const int64_t* qrows;      // table row of every query row of the call, or nullptr
  int64_t r0, n;             // this batch: query rows r0 .. r0 + n - 1
  const float* Y;            // items, ld = Dp
  int Dp;
  int k, pool;               // 1 <= k <= pool <= 1024
  const int32_t* pool_items;   // [n][pool], sorted by the approximate score
  const float* pool_scores;    // [n][pool]
  const unsigned long long* stats;  // launch_two_stage_convert's, of the item table
  int32_t* out_items;        // [n][k]
  float* out_scores;         // [n][k]
  uint8_t* certified;        // [n]
};
hipError_t launch_two_stage_select(const TwoStageSelectArgs& a, hipStream_t s);

// The thin-query scan (audience.hip): the k best eligible rows of a table Y
// for each of a few query rows of X, by recommend.hip's word (score_key(score)
// << 32 | ~id) and its score, the chain acc = fmaf(X[q][c], Y[u][c], acc), c
// ascending from +0 over the padded dim.  thin_scan_kernel holds
// audience_queries_per_pass() queries on chip and reads every row of its
// split of Y once per pass; grid (passes of the batch) x (splits).  A split's
// lists are cut to their best k, then aud_reduce_kernel takes the k best of
// groups of audience_group(k) lists per round until one list is left, which
// rec_merge_kernel writes out.  Eligibility as in RecommendArgs.
struct AudienceArgs {
  const float* X;            // query table, ld = Dp
  const int64_t* qrows;      // table row of every query of the call, or nullptr
  int64_t r0, n;             // this batch: queries r0 .. r0 + n - 1
  const float* Y;            // the table searched, ld = Dp
  int64_t m;                 // its rows
  int Dp;
  int k;                     // 1 .. 1024
  int splits;                // 1 .. chunks of audience_chunk_rows() rows
  const int64_t* row_ptr;    // CSR of the query table's side, or nullptr (no exclusion)
  const int32_t* col;
  const uint32_t* maskw;     // [recommend_words(m)] eligibility bits of Y's rows
  uint32_t* bitmap;          // [n][recommend_words(m)] history bits (workspace), or nullptr
  unsigned long long* cand;  // [n][splits][audience_slots(k)] candidates (workspace)
  int32_t* counts;           // [n][splits] (workspace)
  unsigned long long* red;   // [n][audience_reduce_lists(splits, k)][k] (workspace), or nullptr
  int32_t* red_counts;       // [n][audience_reduce_lists(splits, k)]
  int32_t* out_items;        // [n][k]
  float* out_scores;         // [n][k]
};
int audience_queries_per_pass();
int audience_chunk_rows();
// Candidate slots per (query, split): k + a chunk, rounded up to a power of two.
int audience_slots(int k);
// Lists per group of a reduce round (a group's lists, k rounded up to a power
// of two each, fill the kernel's LDS), the lists the first round leaves (0: one
// split, no round), and the kernels behind the scan, the write-out included.
int audience_group(int k);
int audience_reduce_lists(int splits, int k);
int audience_merge_rounds(int splits, int k);
hipError_t launch_audience_thin(const AudienceArgs& a, hipStream_t s);

// Exact positions of ground-truth items among all eligible items
// (positions.hip): for query row i of the batch and entry t of its ground
// truth gt[gt_ptr[r0 + i] - gt_base .. gt_ptr[r0 + i + 1] - gt_base), rank[t] =
// the number of eligible items whose word (score_key(score) << 32 | ~id) is
// larger than the entry's, -1 when the entry's item is not eligible;
// eligible[i] = the eligible count; mrr / auc as frecsys_position_metrics
// defines them.  Rows, eligibility and scores as in RecommendArgs.  Entry
// regions are indexed by gt_ptr[...] - gt_base; row i's counters start at
// that offset + i (one more counter than entries per row).
struct PositionsArgs {
  const float* X;            // query table, ld = Dp
  const int64_t* qrows;      // table row of every query row of the call, or nullptr
  int64_t r0, n;             // this batch: query rows r0 .. r0 + n - 1
  const float* Y;            // items, ld = Dp
  int64_t m;                 // items
  int Dp;
  int splits;                // item splits, 1 .. positions_max_splits(m)
  const int64_t* row_ptr;    // CSR of the query table's side (with bitmap), or nullptr
  const int32_t* col;
  const uint32_t* maskw;     // [recommend_words(m)] eligibility bits of the items
  uint32_t* bitmap;          // [n][recommend_words(m)] history bits (workspace), or nullptr
  const int64_t* gt_ptr;     // [rows of the call + 1]
  int64_t gt_base;           // gt_ptr[r0]: gt[0] is the first entry of the batch
  const int32_t* gt;         // the batch's ground-truth ids, each in [0, m)
  unsigned long long* words;  // [entries] word per entry, 0 = not eligible (workspace)
  unsigned long long* thr;    // [entries] per row: distinct words, descending (workspace)
  int32_t* g;                // [n] thresholds per row (workspace)
  uint32_t* counters;        // [entries + n] (workspace)
  int32_t* rank;             // [entries]
  int32_t* eligible;         // [n]
  float* mrr;                // [n]
  float* auc;                // [n]
};
hipError_t launch_positions(const PositionsArgs& a, hipStream_t s);
// Thresholds per row that pos_scan_kernel keeps in LDS (longer rows count in
// global memory), and its largest split count: one 128-item tile per split.
int positions_lds_thresholds();
int positions_max_splits(int64_t m);
// Inverse row norms of a table (similar.hip): n2 = the chain acc = fmaf(T[r][c],
// T[r][c], acc), c ascending from +0 over the padded dim -- recommend.hip's
// score of row r with itself, bit for bit -- and inv[r] = n2 > 0 ?
// 1 / sqrt(n2) : 0, sqrt and division correctly rounded.  A function of row r
// alone.
hipError_t launch_row_inv_norm(const float* T, int64_t m, int Dp, float* inv, hipStream_t s);

// Greedy MMR re-ranking of a pool per row (diversify.hip; the semantics are
// frecsys_mmr_select's in include/frecsys_hip.h, to the bit).  Row i has the
// slots ids[i*pool .. i*pool+pool) (negative: empty; repeats are slots of
// their own) with the scores pool_scores[...].  launch_diversify_gram writes
// G[i] = T T^T over the slots' item rows (an empty slot: a zero row), every
// element the chain acc = fmaf(Y[a][c], Y[b][c], acc), c ascending from +0
// over the padded dim; launch_diversify_select reads it and writes the k
// selected ids, their pool scores and (unless out_mmr is null) their MMR
// values, -1 / -FLT_MAX / -FLT_MAX beyond the filled count.
constexpr int kDiversifyMaxPool = 1024;
struct DiversifyArgs {
  const float* Y;            // items, ld = Dp
  int Dp;
  int64_t n;                 // rows of this batch
  int pool;                  // slots per row, 1 .. kDiversifyMaxPool
  int k;                     // 1 .. pool
  float lam;                 // in [0, 1]
  int raw;                   // != 0: rel = score (FRECSYS_DIV_RAW_SCORES)
  const int32_t* ids;        // [n][pool], each negative or in [0, items)
  const float* pool_scores;  // [n][pool]
  float* G;                  // [n][pool][pool] (workspace), or nullptr with lazy
  int lazy;                  // != 0: no Gramian, its rows computed per step by the selection
  int32_t* out_items;        // [n][k]
  float* out_scores;         // [n][k]
  float* out_mmr;            // [n][k], or nullptr
};
hipError_t launch_diversify_gram(const DiversifyArgs& a, hipStream_t s);
hipError_t launch_diversify_select(const DiversifyArgs& a, hipStream_t s);

// Greedy DPP re-ranking of a pool per row (dpp.hip; the semantics are
// frecsys_dpp_select's in include/frecsys_hip.h, to the bit).  The pools and
// G are DiversifyArgs' (launch_diversify_gram writes G); launch_dpp_select
// writes the k selected ids, their pool scores and (unless out_gain is null)
// their gains, -1 / -FLT_MAX / -FLT_MAX beyond the filled count.  The factor
// C, [k][pool] fp32 per row, lies in LDS when dpp_factor_in_lds(pool, k) and
// C is null, else at C (which may be given at any shape); where it lies
// changes no output bit.
constexpr int kDppLdsBytes = 40 * 1024;  // of the CU's 160 KiB: four rows (waves) per CU at the limit
struct DppArgs {
  int64_t n;                 // rows of this batch
  int pool;                  // slots per row, 1 .. kDiversifyMaxPool
  int k;                     // 1 .. pool
  float theta;               // finite, >= 0
  float eps;                 // in (0, 1]
  int raw;                   // != 0: rel = score (FRECSYS_DIV_RAW_SCORES)
  const int32_t* ids;        // [n][pool], each negative or in [0, items)
  const float* pool_scores;  // [n][pool]
  const float* G;            // [n][pool][pool]
  float* C;                  // [n][k][pool] (workspace), or nullptr: LDS
  int32_t* out_items;        // [n][k]
  float* out_scores;         // [n][k]
  float* out_gain;           // [n][k], or nullptr
};
size_t dpp_factor_bytes(int pool, int k);  // 4 k pool
bool dpp_factor_in_lds(int pool, int k);   // dpp_factor_bytes <= kDppLdsBytes
hipError_t launch_dpp_select(const DppArgs& a, hipStream_t s);

// dpp_exp2 of include/frecsys_hip.h: 2^x for |x| <= 64 as a fixed sequence of
// fp32 operations, the same on the host and on the device (rintf in the
// default rounding mode, an exact subtraction, seven explicit fmas over the
// coefficients ln(2)^i / i! rounded to fp32, an exact scaling).
__host__ __device__ inline float dpp_exp2(float x) {
  const float n = rintf(x);
  const float f = x - n;
  float q = 0x1.ffcbfcp-17f;
  q = fmaf(q, f, 0x1.430912p-13f);
  q = fmaf(q, f, 0x1.5d87fep-10f);
  q = fmaf(q, f, 0x1.3b2ab6p-7f);
  q = fmaf(q, f, 0x1.c6b08ep-5f);
  q = fmaf(q, f, 0x1.ebfbe0p-3f);
  q = fmaf(q, f, 0x1.62e430p-1f);
  q = fmaf(q, f, 1.0f);
  return ldexpf(q, (int)n);
}

// Scores of caller-supplied pairs and rankings of caller-supplied candidate
// lists (rerank.hip).  Every score is the chain acc = fmaf(y[c], x[c], acc),
// c ascending from +0 over the padded dim: recommend.hip's score of that row
// and item, bit for bit.
struct ScorePairsArgs {
  const float* X;        // query table, ld = Dp
  const float* Y;        // items, ld = Dp
  int Dp;
  int64_t n;             // pairs of this batch
  const int64_t* rows;   // [n] table row of X per pair
  const int32_t* items;  // [n] item per pair
  float* out;            // [n]
};
hipError_t launch_score_pairs(const ScorePairsArgs& a, hipStream_t s);
// Query row i of the batch (row qrows[r0 + i] of X, or r0 + i) ranks the
// DISTINCT eligible ids of cand[cand_ptr[r0 + i] - cand_base ..
// cand_ptr[r0 + i + 1] - cand_base): the k best by (score descending, id
// ascending), -1 / -FLT_MAX beyond their count.  Eligibility as in
// RecommendArgs: maskw, and bitmap (filled here from row_ptr / col) if given.
struct RankCandArgs {
  const float* X;
  const int64_t* qrows;
  int64_t r0, n;
  const float* Y;
  int64_t m;
  int Dp;
  int k;                     // 1 .. 1024
  const int64_t* cand_ptr;   // [rows of the call + 1]
  const int32_t* cand;       // the batch's candidate ids, each in [0, m)
  int64_t cand_base;         // cand_ptr[r0]: cand[0] is the first id of the batch
  const int64_t* row_ptr;    // CSR of the query table's side (with bitmap), or nullptr
  const int32_t* col;
  const uint32_t* maskw;     // [recommend_words(m)]
  uint32_t* bitmap;          // [n][recommend_words(m)] (workspace), or nullptr
  int32_t* out_items;        // [n][k]
  float* out_scores;         // [n][k], or nullptr
};
hipError_t launch_rank_candidates(const RankCandArgs& a, hipStream_t s);
// Candidates per chunk and candidate words kept in LDS by rank_cand_kernel.
int rank_cand_chunk();
int rank_cand_slots();

// Recall@K / NDCG@K of ranked lists in device memory (metrics.hip): query row
// i of the batch has the list lists[i*k .. i*k+k) (-1 = empty slot, never a
// hit) and the ground truth gt[gt_ptr[r0+i] .. gt_ptr[r0+i+1]) -- ascending,
// distinct, not empty.  gain[j] = 1 / log2(j + 2) and its sequential prefix
// idcg[m] = gain[0] + ... + gain[m-1] are the host's tables (double), so that
// the results are frecsys_list_metrics' bit for bit.
constexpr int kMetricMaxK = 1024;      // largest cut-off (frecsys_recommend's k limit)
constexpr int kMetricMaxCutoffs = 32;  // cut-offs per call (one lane each)
struct RankMetricsArgs {
  const int32_t* lists;     // [n][k]
  int64_t r0, n;            // this batch: query rows r0 .. r0 + n - 1
  int k;                    // list length = max k_list, 1 .. kMetricMaxK
  const int64_t* gt_ptr;    // [rows of the call + 1]
  const int32_t* gt;
  const int32_t* k_list;    // [nk], each 1 .. k
  int nk;                   // 1 .. kMetricMaxCutoffs
  const double* gain;       // [kMetricMaxK]
  const double* idcg;       // [kMetricMaxK + 1]
  float* recall;            // [n][nk]
  float* ndcg;              // [n][nk]
};
hipError_t launch_rank_metrics(const RankMetricsArgs& a, hipStream_t s);

// List quality of ranked lists in device memory (quality.hip; the definitions
// are frecsys_list_quality's in include/frecsys_hip.h).  Row i of the batch has
// the slots lists[i*list_k .. i*list_k+k) (negative: empty; a repeated id is a
// slot of its own), each id below the table's rows.  launch_quality writes, per
// row and cut-off, ILD (float64 running sum over the item rows, ld = Dp) and
// novelty (the mean of weight[id] over the filled slots) -- either output may
// be nullptr, not both; launch_exposure adds 1 to counts[q][id] for every
// filled slot below cut-off q (the caller zeroes counts).
struct QualityArgs {
  const float* Y;         // items, ld = Dp (with ild)
  int Dp;
  const int32_t* lists;   // [n][list_k]
  int64_t n;              // rows of this batch
  int list_k;             // slots per row in memory, >= k
  int k;                  // slots swept = max k_list, 1 .. kMetricMaxK
  const int32_t* k_list;  // [nk], each 1 .. k
  int nk;                 // 1 .. kMetricMaxCutoffs
  const float* weight;    // [items] (with novelty), or nullptr
  float* ild;             // [n][nk], or nullptr
  float* novelty;         // [n][nk], or nullptr
};
struct ExposureArgs {
  const int32_t* lists;   // [n][list_k]
  int64_t n;
  int list_k, k;
  const int32_t* k_list;  // [nk]
  int nk;
  int64_t m;              // items
  unsigned long long* counts;  // [nk][m]
};
hipError_t launch_quality(const QualityArgs& a, hipStream_t s);
hipError_t launch_exposure(const ExposureArgs& a, hipStream_t s);

// Candidate lists of sampled evaluation (sampled.hip): the list of query row
// i of the batch -- cand[cand_ptr[r0 + i] - cand_base ..), RankCandArgs'
// layout -- is the row's ground truth gt[gt_ptr[r0 + i] .. gt_ptr[r0 + i + 1])
// (ascending, distinct) followed by its negatives: the whole pool (every id
// with its maskw bit set that is neither in the ground truth nor, with
// row_ptr / col given, in the row's history; ascending) when 2 n_neg > E or
// 64 E < M, else the first n_neg accepted draws of the generator of
// frecsys_sample_negatives, in draw order.  launch_sampled_pool zeroes the
// batch's bitmaps, sets the blocked bits and writes E = pool[r0 + i];
// launch_sampled_fill writes the lists (their lengths, g + E or g + n_neg, are
// the caller's, from pool[]) and leaves the taken bits set in the bitmaps.
// *fail (~0ull = none) is lowered to r0 + i + 1 for a row that reached the
// draw cap or whose list length does not fit its pool.
constexpr unsigned long long kSampleCapBase = 1ull << 20;  // draws of a sampled row:
constexpr unsigned long long kSampleCapPerNeg = 4096;      // < base + per_neg * n_neg
struct SampledArgs {
  const int64_t* qrows;      // table row of every query row of the call, or nullptr
  int64_t r0, n;             // this batch: query rows r0 .. r0 + n - 1
  int64_t m, W;              // items, recommend_words(m)
  const int64_t* row_ptr;    // CSR of the query table's side, or nullptr (no exclusion)
  const int32_t* col;
  const uint32_t* maskw;     // [W] eligibility bits of the items
  const int32_t* dlist;      // [M] ascending ids with their bit set, or nullptr (M == m)
  int64_t M;
  const int64_t* gt_ptr;     // [rows of the call + 1]
  const int32_t* gt;
  int32_t n_neg;
  unsigned long long seed;
  uint32_t* bitmap;          // [n][W] (workspace)
  int32_t* pool;             // [rows of the call]
  const int64_t* cand_ptr;   // [rows of the call + 1] (fill only)
  int64_t cand_base;
  int32_t* cand;
  unsigned long long* fail;
};
hipError_t launch_sampled_pool(const SampledArgs& a, hipStream_t s);
hipError_t launch_sampled_fill(const SampledArgs& a, hipStream_t s);

// Wide dims, Dp = 512 / 1024 (wide.hip).  d-space solve with A in an HBM
// workspace ([batch][wide_slot_floats(Dp)]), entities a.order[0..n_rows)
// in batches; Gramian by 128x128 block pairs; per-step tridiagonalisation
// (work: wide_tridiag_work_floats); rotations; user loss (a.quad holds
// wide_quad_floats partials).
bool wide_dim(int Dp);
size_t wide_slot_floats(int Dp);
// Long-history split of the wide d-space SYRK: entities of the first batch
// with more than 2 * wide_slab_rows() assembly rows have their SYRK cut into
// slabs of wide_slab_rows() (the two-level accumulation block, so the slab
// sums fold into exactly the unsplit result) in a.work / a.split / a.slabs
// ([slabs][wide_slab_floats(Dp)]), computed by their own workgroups first.
int64_t wide_slab_rows();
size_t wide_slab_floats(int Dp);
int64_t wide_rows_per_leaf(int64_t n);
// Leaves of g (rows [g.row0, g.row0 + g.n), leaf size g.plan.rpl) into g.partials.
hipError_t launch_wide_gram_leaves(int Dp, const GramArgs& g, hipStream_t s);
hipError_t launch_wide_gram_final(int Dp, const float* gslabs, int64_t ngroup, float* G,
                                  hipStream_t s);
// xsplit: a buffer of wide_xsplit_bytes(Dp, a.n_other) (wide.h) for the SYRK
// from the pre-split table, or nullptr for the register-staged SYRK
hipError_t launch_wide_solve(int Dp, const SolveArgs& a, float* ws, int64_t batch,
                             hipStream_t s, char* xsplit = nullptr);
size_t wide_tridiag_work_floats(int Dp);
bool wide_tridiag_tagged();
hipError_t launch_wide_tridiag(const float* G, int Dp, float* tdiag, float* toff, float* Vh,
                               float* tau, float* work, hipStream_t s, float* Q = nullptr,
                               void* img_q = nullptr, void* img_qt = nullptr,
                               unsigned* tcount = nullptr);
size_t wide_quad_floats(int Dp, int64_t rows);
hipError_t launch_wide_user_loss(int Dp, const LossArgs& a, hipStream_t s);
hipError_t launch_user_loss(int Dp, const LossArgs& a, hipStream_t s);
hipError_t launch_zero_gram(int Dp, float* G, hipStream_t s);
// Train-loss diagnostics: out[r] = ||X[r]||^2 for n rows; dot = sum_ij A_ij B_ij
// (double, Dp x Dp).
hipError_t launch_row_norm2(const float* X, int64_t n, int Dp, float* out, hipStream_t s);
// ||X[r] - Y[r]||^2 per row (the print_residual_stats norms)
hipError_t launch_row_diff2(const float* X, const float* Y, int64_t n, int Dp, float* out,
                            hipStream_t s);
hipError_t launch_gram_dot(const float* A, const float* B, int Dp, double* dot, hipStream_t s);

// Padded leading dimension for a logical dimension (8, 16, multiples of 32
// up to 256, then 512 and 1024).  Returns 0 when unsupported.
int padded_dim(int dim);
// true (default): the SYRK kernels run fp32-accurate split-bf16 MFMA
// (common.h mfma_x6); FRECSYS_SYRK_F32=1 selects v_mfma_f32_32x32x2_f32.
bool syrk_split_bf16();
// true when a gather over `rows` rows of ld Dp needs 64-bit element offsets
// (rows * Dp >= 2^32), or FRECSYS_GATHER64=1 forces them (tests: the two
// widths are bit-identical).
bool gather_off64(int64_t rows, int Dp);

}  // namespace frecsys_hip
