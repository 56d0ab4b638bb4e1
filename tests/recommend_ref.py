"""Float64 reference and exact inputs for frecsys_recommend (helper of
tests/test_recommend_cpu.py, tests/test_recommend_gpu.py and
tests/test_recommend_model_gpu.py; not a test).

recommend64()   scores in float64, ineligible items at -inf, the k first by
                (score descending, item id ascending); ids listed at -inf
                become -1.
grid_inputs()   integer-grid tables: every entry of both tables is drawn
                uniformly from {-2..2}, so every score is an integer of
                magnitude <= 4 dim <= 4096 -- exact in fp32 whatever the
                summation order, and exact under 3-piece bf16 splits too (a
                small integer has one non-zero piece).  Heavy ties are the
                point: a streaming top-K goes wrong on them at tile,
                compaction and split edges.
grid_plan()     the cases of the exact GPU test.
"""
import numpy as np

import aux_data as A

GRID_M = (1, 127, 128, 129, 255, 256, 257, 1024, 1025, 5000)
GRID_ROWS = (1, 63, 64, 65)
GRID_DIMS = (5, 20, 64, 200, 500, 1000)
GRID_KINDS = ("one", "k33", "max")  # k = 1, 33, min(items, 1024)
# the kernel's candidate buffer holds 512 (k <= 128), 1024 (k <= 256) or 2048
# slots and is compacted when a further 128-item tile might not fit.  With
# every item eligible, no threshold yet and one item split, item counts of
# 512 / 2048 -1 | 0 | +1 fill the smallest (k = 33) and the largest
# (k = 1024) buffer to its last slot: (m, k)
CAP_EDGE = ((511, 33), (512, 33), (513, 33), (2047, 1024), (2048, 1024), (2049, 1024))


def grid_k(m, kind):
    return {"one": 1, "k33": 33, "max": min(m, 1024)}[kind]


def recommend64(X, V, ptr, col, rows, k, exclude, mask):
    """(S, items, scores): S float64 [n, m] with ineligible items at -inf,
    items int32 [n, k] (-1 where the listed score is -inf or k exceeds the
    item count), scores float64 [n, k] (-inf there).  rows None = every row
    of X.  `+ 0.0` turns a float64 -0.0 into +0.0: an FMA chain from +0 never
    yields -0, and the two differ in their bits."""
    X = np.asarray(X)
    V = np.asarray(V)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows, np.int64)
    S = X[rows].astype(np.float64) @ V.astype(np.float64).T + 0.0
    m = V.shape[0]
    if exclude:
        for i, r in enumerate(rows):
            S[i, col[ptr[r]:ptr[r + 1]]] = -np.inf
    if mask is not None:
        S[:, np.asarray(mask) == 0] = -np.inf
    ids = np.broadcast_to(np.arange(m), S.shape)
    order = np.lexsort((ids, -S), axis=1)[:, :k]
    sc = np.take_along_axis(S, order, axis=1)
    items = np.where(np.isfinite(sc), order, -1).astype(np.int32)
    if k > m:
        pad = k - m
        items = np.concatenate([items, np.full((len(rows), pad), -1, np.int32)], axis=1)
        sc = np.concatenate([sc, np.full((len(rows), pad), -np.inf)], axis=1)
    return S, items, sc


def grid_inputs(m, rows, k, dim, seed):
    """(X, V, ptr, col): float32 integer tables of {-2..2} and the histories
    of aux_data.aux_eval (an empty row, the row {0, m - 1}, repeated ids, a
    row with only k - 1 free items)."""
    rng = np.random.default_rng(seed)
    V = rng.integers(-2, 3, (m, dim)).astype(np.float32)
    X = rng.integers(-2, 3, (rows, dim)).astype(np.float32)
    ptr, col = A.aux_eval(rows, m, k, seed + 1)
    return X, V, ptr, col


def grid_mask(m, kind, seed):
    """None, a mask keeping about 70 % of the items, or all zeros."""
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros(m, np.uint8)
    return (np.random.default_rng(seed + 2).random(m) < 0.7).astype(np.uint8)


def grid_main():
    """(m, rows, k kind, dim, exclude, mask kind, seed): the rotated part of
    grid_plan()."""
    out = []
    for i, m in enumerate(GRID_M):
        for j, dim in enumerate(GRID_DIMS):
            rows = GRID_ROWS[(i + j) % 4]
            kind = GRID_KINDS[(i + 2 * j) % 3]
            exclude = bool((i + j // 2) % 2)
            mask = ("none", "m70")[(i // 2 + j) % 2]
            out.append((m, rows, kind, dim, exclude, mask, 3000 + 10 * i + j))
    return out


def grid_plan():
    """(m, rows, k, dim, exclude, mask kind, splits, seed).  Every item count
    at every dim; rows, k kind, exclude and mask rotated so that every pair of
    values of two parameters occurs (test_recommend_cpu checks the cover);
    splits None = the automatic count.  Then the single cases: k = items + 3,
    the all-zero mask, and with one item split (so that one workgroup sees
    every item) two compactions of the smallest and of the largest buffer and
    the capacity edge."""
    out = [(m, rows, grid_k(m, kind), dim, exclude, mask, None, seed)
           for m, rows, kind, dim, exclude, mask, seed in grid_main()]
    out.append((127, 64, 130, 20, True, "none", None, 3901))    # k = items + 3
    out.append((257, 65, 33, 64, True, "zero", None, 3902))     # nothing eligible
    out.append((5000, 65, 33, 20, True, "none", 1, 3903))       # 512 slots, filled repeatedly
    out.append((5000, 65, 200, 20, False, "none", 1, 3920))     # 1024 slots
    out.append((5000, 65, 1024, 64, False, "m70", 1, 3904))     # 2048 slots, 3,500 eligible
    for e, (m, k) in enumerate(CAP_EDGE):
        out.append((m, 5, k, 5, False, "none", 1, 3905 + e))
    return out
