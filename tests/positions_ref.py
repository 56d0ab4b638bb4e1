"""Reference and exact inputs for frecsys_rank_positions /
frecsys_position_metrics (helper of tests/test_positions_cpu.py,
tests/test_positions_gpu.py and tests/test_positions_model_gpu.py; not a
test).

ranks64()               positions from the S of recommend_ref.recommend64
                        (float64, -inf = ineligible) by (score descending,
                        item id ascending); -1 for an ineligible item; and the
                        eligible count per row.
position_metrics_ref()  mrr / auc in Python ints and float64, cast once to
                        float32.
plan()                  the cases of the exact GPU test, on the integer-grid
                        tables of recommend_ref.grid_inputs (every score exact
                        in fp32 in any order; heavy ties, which is where a count
                        goes wrong).
"""
import itertools

import numpy as np

import recommend_ref as RR

# pos_scan_kernel keeps the thresholds of a row in LDS when the row has at most
# this many (csrc/positions.hip kPosLds); a longer row counts in global memory
LDS_THRESHOLDS = 32
# pos_prepare_kernel sorts up to this many words in LDS, more in global memory
# (csrc/positions.hip kSortLds)
SORT_LDS = 2048

PLAN_M = (1, 127, 128, 129, 257, 1024, 1025, 3000)
PLAN_ROWS = (1, 63, 64, 65)
PLAN_DIMS = (5, 64, 200, 500)
PLAN_EXCLUDE = (False, True)
PLAN_MASK = ("none", "m70", "zero")
PLAN_GT = ("one", "two", "L-1", "L", "L+1", "all")  # ground-truth entries per row
PLAN_SPLITS = (None, 1, 64)
PLAN_AXES = (PLAN_M, PLAN_ROWS, PLAN_DIMS, PLAN_EXCLUDE, PLAN_MASK, PLAN_GT, PLAN_SPLITS)
HIST_K = 33  # aux_eval's k: row 3 keeps 32 items free


def gt_count(m, kind):
    """Entries per row of a ground-truth kind; an int is its own count."""
    if isinstance(kind, int):
        return kind
    return {"one": 1, "two": 2, "L-1": LDS_THRESHOLDS - 1, "L": LDS_THRESHOLDS,
            "L+1": LDS_THRESHOLDS + 1, "all": m}[kind]


def ranks64(S, gt_ptr, gt_items):
    """(rank int32 [gt_ptr[n]], eligible int32 [n])."""
    S = np.asarray(S, np.float64)
    n, m = S.shape
    rank = np.full(int(gt_ptr[n]), -1, np.int32)
    ids = np.arange(m)
    for i in range(n):
        order = np.lexsort((ids, -S[i]))
        pos = np.empty(m, np.int64)
        pos[order] = ids
        g = np.asarray(gt_items[gt_ptr[i]:gt_ptr[i + 1]], np.int64)
        rank[gt_ptr[i]:gt_ptr[i + 1]] = np.where(np.isfinite(S[i, g]), pos[g], -1)
    return rank, np.isfinite(S).sum(axis=1).astype(np.int32)


def position_metrics_ref(rank, gt_ptr, eligible):
    """(mrr, auc) float32 [n]."""
    n = len(gt_ptr) - 1
    mrr = np.zeros(n, np.float32)
    auc = np.zeros(n, np.float32)
    for i in range(n):
        R = sorted({int(r) for r in rank[gt_ptr[i]:gt_ptr[i + 1]] if r >= 0})
        g, M = len(R), int(eligible[i])
        if g == 0:
            continue
        mrr[i] = np.float32(np.float64(1.0) / np.float64(R[0] + 1))
        if M == g:
            auc[i] = np.float32(1.0)
        else:
            inv = sum(r - q for q, r in enumerate(R))
            auc[i] = np.float32(np.float64(1.0) -
                                np.float64(inv) / (np.float64(g) * np.float64(M - g)))
    return mrr, auc


def ground_truth(m, rows, kind, ptr, col, seed):
    """(gt_ptr, gt_items): gt_count entries per row in random order, distinct
    while the items allow (drawn with repeats beyond that); from two entries
    on, the second is the first item of the row's history when it has one (-1
    expected under exclusion), and every fifth row repeats its first entry."""
    rng = np.random.default_rng(seed + 7)
    cnt = gt_count(m, kind)
    out = []
    for r in range(rows):
        g = rng.permutation(m)[:cnt] if cnt <= m else rng.integers(0, m, cnt)
        g = g.astype(np.int32)
        if cnt >= 2 and ptr[r + 1] > ptr[r] and col[ptr[r]] not in g:
            g[1] = col[ptr[r]]
        if r % 5 == 4:
            g = np.concatenate([g, g[:1]])
        out.append(g)
    gp = np.concatenate([[0], np.cumsum([len(g) for g in out])]).astype(np.int64)
    return gp, np.concatenate(out).astype(np.int32)


def inputs(m, rows, dim, gt, seed):
    """(X, V, ptr, col, gt_ptr, gt_items) of a plan case."""
    X, V, ptr, col = RR.grid_inputs(m, rows, HIST_K, dim, seed)
    gp, gi = ground_truth(m, rows, gt, ptr, col, seed)
    return X, V, ptr, col, gp, gi


def _pairs(case):
    return {(a, b, case[a], case[b]) for a, b in itertools.combinations(range(len(case)), 2)}


def plan_main():
    """(m, rows, dim, exclude, mask kind, gt kind, splits): a pairwise cover of
    PLAN_AXES -- every pair of values of two parameters occurs.  Built
    greedily: the best of 40 seeded random candidates per step, until nothing
    is left uncovered; deterministic."""
    rng = np.random.default_rng(20)
    todo = set()
    for a, b in itertools.combinations(range(len(PLAN_AXES)), 2):
        todo |= {(a, b, x, y) for x in PLAN_AXES[a] for y in PLAN_AXES[b]}
    out = []
    while todo:
        first = sorted(todo, key=repr)[0]  # the candidate covers at least this pair
        best, gain = None, -1
        for _ in range(40):
            c = [ax[int(rng.integers(len(ax)))] for ax in PLAN_AXES]
            c[first[0]], c[first[1]] = first[2], first[3]
            gn = len(_pairs(tuple(c)) & todo)
            if gn > gain:
                best, gain = tuple(c), gn
        out.append(best)
        todo -= _pairs(best)
    return out


def plan():
    """(m, rows, dim, exclude, mask kind, gt, splits, seed): plan_main(), then
    the single cases -- ground-truth counts on both sides of the prepare
    kernel's LDS sort limit, and every item as ground truth with one split (one
    workgroup sees every item) and with the most."""
    out = [c + (5000 + i,) for i, c in enumerate(plan_main())]
    for e, cnt in enumerate((SORT_LDS - 1, SORT_LDS, SORT_LDS + 1)):
        out.append((3000, 5, 5, bool(e % 2), "none", cnt, None, 5900 + e))
    out.append((3000, 65, 64, True, "m70", "all", 1, 5910))
    out.append((1025, 64, 200, False, "none", "all", 64, 5911))
    return out
