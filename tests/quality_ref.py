"""Float64 numpy reference and fixtures for the list-quality calls
(frecsys_list_quality, frecsys_exposure_summary, frecsys_lists_quality,
frecsys_rank_quality; helper of tests/test_quality_cpu.py,
tests/test_quality_gpu.py and tests/test_quality_model_gpu.py; not a test).
Does not import the library.

quality64()    ILD, novelty and exposure of lists per cut-off in float64.  ILD is
               computed PAIRWISE -- 1 - the mean of cos(a, b) over all pairs of
               filled slots, from the Gramian of the normalised rows -- not by
               the library's running sum, so a comparison checks the algebra as
               well as the code.
close()        the bound of include/frecsys_hip.h: |a - b| <= 2^-23 max(1, |b|).
               Every sum on either side is float64 (reordering moves it by about
               (K + Dp) 2^-52); what remains is the rounding of the result to
               fp32, half an ulp a side.
summary_exact() coverage and Gini of an exposure row in exact rational
               arithmetic (fractions.Fraction), rounded once.
item_table()   300 (or more) Gaussian item rows scaled over two decades, with one
               all-zero row (ZERO) and two identical rows (TWIN).
caller_lists() lists "from anywhere": the empty list, one and two filled slots,
               one item repeated, the zero row, the twins side by side, empty
               slots in the middle, a short list, random ids with repeats.
"""
from fractions import Fraction

import numpy as np

DIMS = (8, 16, 20, 64, 200, 256, 1000)
M = 300                                  # items of the standard table; list_k of its lists
K300 = (1, 2, 63, 64, 65, 300)
K_UNSORTED = (65, 2, 300, 2, 1)          # any order, a repeat
M_BIG, DIM_BIG, K_BIG = 1100, 64, (5, 1024)   # the K limit
ZERO, TWIN = 7, (20, 21)
BOUND = 2.0 ** -23


def item_table(m, dim, seed):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((m, dim)) * 10.0 ** rng.uniform(-1, 1, (m, 1))
    T = T.astype(np.float32)
    T[ZERO] = 0.0
    T[TWIN[1]] = T[TWIN[0]]
    return T


def item_weights(m, seed):
    """Self-information-like weights: -log2 of a popularity share."""
    rng = np.random.default_rng(seed)
    return (-np.log2(rng.uniform(1e-5, 1.0, m))).astype(np.float32)


def caller_lists(m, list_k, seed, rows=14):
    """int32 [rows, list_k]: the named cases first, random rows behind them."""
    rng = np.random.default_rng(seed)
    L = np.full((rows, list_k), -1, np.int32)
    # 0: no filled slot.  1: one.  2: two, far apart
    L[1, min(3, list_k - 1)] = 5
    L[2, 0], L[2, list_k - 1] = 11, 12
    L[3, :] = 33                                   # one item repeated
    L[4, :] = rng.permutation(m)[:list_k] if list_k <= m else rng.integers(0, m, list_k)
    L[4, 1] = ZERO                                 # the zero row among others
    L[5, :] = rng.integers(0, m, list_k)
    L[5, 0], L[5, 1] = TWIN                        # the identical rows side by side
    L[6, :] = rng.integers(0, m, list_k)
    L[6, rng.random(list_k) < 0.4] = -1            # empty slots in the middle
    L[6, 0] = -1
    short = max(1, list_k // 5)
    L[7, :short] = rng.integers(0, m, short)       # shorter than most cut-offs
    L[8, :] = ZERO                                 # nothing but zero rows
    for i in range(9, rows):
        L[i] = rng.integers(0, m, list_k)
        L[i, rng.random(list_k) < 0.1 * (i - 9)] = -1
    return L


def quality64(T, lists, k_list, weight=None):
    """(ild float64 [n, nk], novelty float64 [n, nk] or None, exposure int64
    [nk, items])."""
    T64 = np.asarray(T, np.float64)
    lists = np.asarray(lists)
    n, nk, m = lists.shape[0], len(k_list), T64.shape[0]
    norm = np.sqrt((T64 * T64).sum(1))
    inv = np.divide(1.0, norm, out=np.zeros_like(norm), where=norm > 0)
    Th = T64 * inv[:, None]
    ild = np.zeros((n, nk))
    nov = None if weight is None else np.zeros((n, nk))
    exposure = np.zeros((nk, m), np.int64)
    for q, K in enumerate(k_list):
        for i in range(n):
            ids = lists[i, :K]
            ids = ids[ids >= 0]
            cnt = len(ids)
            exposure[q] += np.bincount(ids, minlength=m)
            if cnt >= 2:
                G = Th[ids] @ Th[ids].T
                pairs = cnt * (cnt - 1) // 2
                ild[i, q] = 1.0 - np.triu(G, 1).sum() / pairs
            if nov is not None and cnt >= 1:
                nov[i, q] = np.asarray(weight, np.float64)[ids].sum() / cnt
    return ild, nov, exposure


def close(got, ref):
    """The worst |a - b| / max(1, |b|) in units of the bound (<= 1 passes)."""
    a = np.asarray(got, np.float64)
    b = np.asarray(ref, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) / BOUND)


def summary_exact(counts, mask=None):
    """{"coverage", "gini", "total", "covered"} with the two ratios formed in
    exact rational arithmetic and rounded once to float64."""
    c = [int(x) for i, x in enumerate(counts) if mask is None or mask[i]]
    M_, S = len(c), sum(c)
    covered = sum(1 for x in c if x > 0)
    if M_ == 0 or S == 0:
        return {"coverage": 0.0, "gini": 0.0, "total": S, "covered": covered}
    c.sort()
    num = sum((2 * (i + 1) - M_ - 1) * x for i, x in enumerate(c))
    return {"coverage": float(Fraction(covered, M_)), "gini": float(Fraction(num, M_ * S)),
            "total": S, "covered": covered}
