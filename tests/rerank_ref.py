"""Float64 reference and exact inputs for frecsys_rank_candidates /
frecsys_score_pairs (helper of tests/test_rerank_cpu.py,
tests/test_rerank_gpu.py and tests/test_rerank_model_gpu.py; not a test).

rank64()       per query row the DISTINCT eligible ids of its candidate list,
               scored in float64 (`+ 0.0`: an FMA chain from +0 never yields
               -0), the k first by lexsort((ids, -S)); -1 / -inf beyond them.
grid_plan()    the cases of the exact GPU test, on recommend_ref.grid_inputs'
               integer tables (entries in {-2..2}: every score an exact fp32
               integer, heavy ties).  One call mixes every list length of
               GRID_LENS over its rows.
grid_lists()   the candidate lists of a case.
gauss_lists()  the lists of the Gaussian test and the rows its gap condition
               flags.
"""
import numpy as np

import recommend_ref as RR

# Every power-of-two edge up to 8192 (any power-of-two chunk or buffer size is
# hit: the kernel sweeps 256 candidates per chunk and keeps 2048 words), the
# kernel's cut point 1792 = 2048 - 256 (a buffer holding more is sorted and cut
# before the next chunk), k - 1 | k | k + 1 ("k-1", "k", "k+1": resolved per
# case), the empty list, and 20,000: longer than either catalogue.
GRID_LENS = (0, 1, 63, 64, 65, 127, 128, 129, "k-1", "k", "k+1", 255, 256, 257, 511, 512, 513,
             1023, 1024, 1025, 1791, 1792, 1793, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192,
             8193, 20000)
GRID_KS = (1, 33, 1024)
GRID_DIMS = RR.GRID_DIMS          # (5, 20, 64, 200, 500, 1000): every padded-dim class
GRID_M = (129, 5000)
GRID_ROWS = (63, 65)              # both hold every length class; 1 row: the singles


def rank64(X, V, ptr, col, rows, cand_ptr, cand_items, k, exclude, mask):
    """(items int32 [n, k], scores float64 [n, k]): list i ranked for row
    rows[i] of X (rows None: row i)."""
    X = np.asarray(X)
    V64 = np.asarray(V).astype(np.float64)
    cand_ptr = np.asarray(cand_ptr, np.int64)
    cand_items = np.asarray(cand_items)
    n = len(cand_ptr) - 1
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    items = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), -np.inf)
    for i, r in enumerate(rows):
        ids = np.unique(cand_items[cand_ptr[i]:cand_ptr[i + 1]]).astype(np.int64)
        if mask is not None:
            ids = ids[np.asarray(mask)[ids] != 0]
        if exclude:
            ids = ids[~np.isin(ids, col[ptr[r]:ptr[r + 1]])]
        S = V64[ids] @ X[r].astype(np.float64) + 0.0
        order = np.lexsort((ids, -S))[:k]
        items[i, :len(order)] = ids[order]
        scores[i, :len(order)] = S[order]
    return items, scores


def grid_len(L, k):
    return {"k-1": k - 1, "k": k, "k+1": k + 1}.get(L, L)


def grid_lists(m, lens, seed):
    """(cand_ptr, cand_items): list i has lens[i] ids drawn with replacement
    from [0, m) -- repeats everywhere, and a list longer than m holds most of
    the catalogue several times --, then one id three times in a row in the
    middle and the id of position 0 again at position len - 1 (chunks apart in
    a long list)."""
    rng = np.random.default_rng(seed)
    out = []
    for L in lens:
        c = rng.integers(0, m, L).astype(np.int32)
        if L >= 5:
            c[L // 2:L // 2 + 3] = c[L // 2]
        if L >= 2:
            c[L - 1] = c[0]
        out.append(c)
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in out])]).astype(np.int64)
    ids = np.concatenate(out).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, ids


def case_lens(rows, k, shift):
    """The list length of every row: GRID_LENS in order from `shift` on."""
    L = len(GRID_LENS)
    return [grid_len(GRID_LENS[(i + shift) % L], k) for i in range(rows)]


def grid_main():
    """(m, rows, k, dim, exclude, mask kind, shift, seed): every (k, dim)
    pair; rows >= len(GRID_LENS), so every case holds every length class."""
    out = []
    for a, k in enumerate(GRID_KS):
        for b, dim in enumerate(GRID_DIMS):
            m = GRID_M[(a + b) % 2]
            rows = GRID_ROWS[(a + b // 2) % 2]
            exclude = bool((a + b // 3) % 2)
            mask = ("none", "m70")[(a + b // 2 + b) % 2]
            out.append((m, rows, k, dim, exclude, mask, 5 * a + 7 * b, 7000 + 10 * a + b))
    return out


def grid_plan():
    """grid_main(), then the singles: one row (the empty list, the longest
    list, one past two full buffers), and the all-zero mask."""
    out = grid_main()
    L = list(GRID_LENS)
    out.append((129, 1, 33, 20, True, "none", L.index(0), 7901))
    out.append((5000, 1, 1024, 64, False, "m70", L.index(20000), 7902))
    out.append((5000, 1, 1, 200, False, "none", L.index(4097), 7903))
    out.append((129, 65, 33, 5, True, "zero", 3, 7904))
    return out


def grid_case(m, rows, k, dim, exclude, mk, shift, seed):
    """(X, V, ptr, col, mask, cand_ptr, cand_items) of a plan entry."""
    X, V, ptr, col = RR.grid_inputs(m, rows, k, dim, seed)
    mask = RR.grid_mask(m, mk, seed)
    cp, ci = grid_lists(m, case_lens(rows, k, shift), seed + 3)
    return X, V, ptr, col, mask, cp, ci


# ---- Gaussian lists ----
GAUSS_LEN = 300
# (aux_data.topk_cases() entry, list seed).  First the case
# test_recommend_gpu.test_gaussian_float64 runs per item count (its bar is the
# one taken over), or, where the float64 ranking of 300-id lists alone flags
# more than 5 % of its rows under each of the list seeds case seed + 500 .. 503
# (k = 256 .. 1024 of 63 .. 65 rows), the next case of that item count in plan
# order; the list seed is the first of the four that stays under the limit
# (tests/test_rerank_cpu.py counts).  Then further cases with k = 33 and
# k >= the distinct count on more than one row, under the same limit.
# The bar's scale max|S| is taken over the whole catalogue: at one item it is
# the largest of 65 scores only, and the dim-200 case (1, 65, 1, 200) misses
# it with recommend's own bits (2.78e-7 against 2.73e-7), so the item count 1
# keeps test_recommend_gpu's case.
GAUSS_CASES = (
    ((1, 1, 1, 5, 1000), 1500), ((127, 64, 1, 20, 1011), 1511),
    ((128, 1, 1, 64, 1022), 1522), ((129, 64, 1, 200, 1033), 1533),
    ((255, 1, 1, 500, 1044), 1544), ((256, 64, 33, 20, 1051), 1551),
    ((257, 65, 257, 20, 1061), 1562), ((1024, 64, 33, 200, 1073), 1573),
    ((1025, 1, 33, 500, 1084), 1584),
    ((127, 65, 127, 64, 1012), 1513), ((129, 65, 129, 500, 1034), 1534),
    ((255, 65, 33, 200, 1043), 1546), ((1025, 1, 1024, 5, 1080), 1580),
    ((1025, 63, 33, 20, 1081), 1584),
)


def gauss_lists(m, rows, seed):
    """`rows` lists of GAUSS_LEN ids drawn with replacement from [0, m)."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, m, (rows, GAUSS_LEN)).astype(np.int32)
    ptr = (GAUSS_LEN * np.arange(rows + 1)).astype(np.int64)
    return ptr, ids.reshape(-1)


def gauss_flagged(sc, tol):
    """Rows whose float64 ranking has two listed-or-boundary scores closer
    than 2 tol: sc [n, k + 1] from rank64(.., k + 1, ..) (the k listed and the
    boundary; -inf = empty slot, never flags)."""
    with np.errstate(invalid="ignore"):
        gap = sc[:, :-1] - sc[:, 1:]
    fin = np.isfinite(sc[:, :-1]) & np.isfinite(sc[:, 1:])
    return np.any(fin & (gap < 2.0 * tol), axis=1)
