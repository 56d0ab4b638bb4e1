"""Ground truth, CVaR and float64 metric references for the evaluate API
(helper of tests/test_metrics_cpu.py, tests/test_metrics_gpu.py and
tests/test_evaluate_model_gpu.py; not a test).

ground_truth()  one non-empty ground-truth row per query row, disjoint from
                the row's history unless asked otherwise, with the rows a
                metric kernel can go wrong on.
cvar_ref()      EvaluationResult::cvar (evaluation.h:83-102) in sequential
                np.float32 arithmetic, quirks included.
metrics64()     Recall@K / NDCG@K restated plainly in float64 (for error
                messages and hand-written cases; no bitwise claim).
"""
import numpy as np

K_LISTS = ((1,), (5, 10, 20, 50, 100), (63, 64, 65), (1024, 1, 128, 128))
GRID_M = (127, 130, 1025)
GRID_ROWS = (1, 5, 65)
GRID_DIM = 20
DEFAULT_ALPHAS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)


def grid_cases():
    """(m, rows, k_list, seed) of the exact tests: every item count with every
    row count and every cut-off list, then m = 127 with the cut-off 130 (a
    list padded with -1)."""
    out = []
    for i, m in enumerate(GRID_M):
        for j, rows in enumerate(GRID_ROWS):
            for q, ks in enumerate(K_LISTS):
                out.append((m, rows, ks, 4100 + 100 * i + 10 * j + q))
    out.append((127, 5, (130,), 4500))
    return out


def ground_truth(rows, m, ptr, col, seed, kmax=100, disjoint=True):
    """(gt_ptr int64 [n + 1], gt_items int32) for the query rows `rows` (side
    row ids, or a count n = rows 0 .. n-1) of a side with the CSR histories
    ptr / col over m items.  Every row is non-empty and, with disjoint, holds
    no item of its own history (a row whose history is every item gets
    {m - 1}).  Query row 0: {0, m - 1} (what of it is free); 1: one item; 2:
    repeated ids; 3: 70 distinct ids (more than one 64-bit word of a binary
    search) where m allows; 4: kmax + 5 ids (longer than the largest cut-off)
    where m allows; the others 1..40 distinct ids.  Ids are in drawn order, not
    sorted.  Without disjoint, every row also gets up to three items of its
    history."""
    rows = np.arange(rows) if np.isscalar(rows) else np.asarray(rows, np.int64)
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(rows):
        hist = np.asarray(col[ptr[r]:ptr[r + 1]], np.int64)
        free = np.setdiff1d(np.arange(m), hist) if disjoint else np.arange(m)
        if len(free) == 0:
            g = [m - 1]
        elif i == 0:
            g = [x for x in (0, m - 1) if x in free] or [free[0]]
        elif i == 1:
            g = [rng.choice(free)]
        elif i == 2:
            a = rng.choice(free, min(6, len(free)), replace=False)
            g = np.concatenate([a, a[:3], a[1:2]])
        elif i == 3:
            g = rng.choice(free, min(70, len(free)), replace=False)
        elif i == 4:
            g = rng.choice(free, min(kmax + 5, len(free)), replace=False)
        else:
            g = rng.choice(free, min(int(rng.integers(1, 41)), len(free)), replace=False)
        g = np.asarray(g, np.int32)
        if not disjoint and len(hist):
            g = np.concatenate([g, hist[:3].astype(np.int32)])
        out.append(g)
    gp = np.concatenate([[0], np.cumsum([len(g) for g in out])]).astype(np.int64)
    return gp, np.concatenate(out).astype(np.int32)


def cvar_ref(values, alphas):
    """evaluation.h:83-102: the ascending sort, the sequential fp32 running
    sum, and the scan `for (j = counter; j < na; ++j)` in which a match writes
    out[counter++] -- so results land in match order, an alpha with
    int(n * alpha) >= n leaves a zero, and so do the later ones of an unsorted
    list."""
    ms = np.sort(np.asarray(values, np.float32))
    al = np.asarray(alphas, np.float32)
    out = np.zeros(len(al), np.float32)
    n = len(ms)
    counter = 0
    acc = np.float32(0.0)
    for i in range(n):
        acc = np.float32(acc + ms[i])
        j = counter
        while j < len(al):
            if int(np.float32(np.float32(n) * al[j])) == i:
                out[counter] = np.float32(acc / np.float32(i + 1))
                counter += 1
            j += 1
    return out


def metrics64(lists, gt_ptr, gt_items, k_list):
    """(recall, ndcg) float64 [n, nk], plainly."""
    lists = np.asarray(lists)
    n, list_k = lists.shape
    rec = np.zeros((n, len(k_list)))
    ndcg = np.zeros((n, len(k_list)))
    for i in range(n):
        gt = set(int(x) for x in gt_items[gt_ptr[i]:gt_ptr[i + 1]])
        for q, k in enumerate(k_list):
            hit = [j for j in range(min(int(k), list_k)) if int(lists[i, j]) in gt]
            dcg = sum(1.0 / np.log2(j + 2.0) for j in hit)
            norm = sum(1.0 / np.log2(j + 2.0) for j in range(min(int(k), len(gt))))
            rec[i, q] = len(hit) / min(int(k), len(gt))
            ndcg[i, q] = dcg / norm
    return rec, ndcg
