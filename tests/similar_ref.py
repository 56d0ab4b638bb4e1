"""Float64 reference, exact inputs and case plans for frecsys_similar (helper
of tests/test_similar_cpu.py, tests/test_similar_gpu.py and
tests/test_similar_model_gpu.py; not a test).

similar64()     scores of rows of ONE table against that table in float64 (dot
                product or cosine; a zero row has cosine 0 with everything),
                ineligible rows and -- without keep_self -- the query's own id
                at -inf, the k first by (score descending, id ascending); ids
                listed at -inf become -1.  recommend_ref.recommend64's
                conventions.
grid_table()    recommend_ref.grid_inputs' item table: entries uniform in
                {-2..2}, every dot an exact integer with heavy ties.
sign_table()    entries +-1: every squared norm is dim exactly, so every
                inverse norm is one and the same float; optionally rows 0 and
                m - 1 all zero.
gauss_table()   Gaussian rows, each scaled by 10^u with u uniform in
                [-1.5, 1.5]: norms over three decades, so that the dot order
                and the cosine order differ.
query_rows()    the query ids of a case.
dot_plan(), cosine_plan(), gauss_plan()   the cases of the GPU tests.
check_cosine()  the tolerant rule of the float64 comparison.
"""
import numpy as np

import recommend_ref as RR

USER, ITEM = 0, 1   # frecsys_hip.SIDE_USER / SIDE_ITEM

GRID_M = (1, 2, 127, 128, 129, 257, 513, 1025, 5000)
GRID_ROWS = (1, 63, 64, 65)
GRID_DIMS = (5, 64, 200, 500)
GRID_KINDS = ("one", "k33", "max")   # k = 1, 33, min(m, 1024)
GAUSS_M = (129, 1025, 5000)
GAUSS_DIMS = (20, 256, 1000)
GAUSS_KS = (10, 200)


def grid_k(m, kind):
    return {"one": 1, "k33": 33, "max": min(m, 1024)}[kind]


def similar64(T, rows, k, cosine, keep_self, mask):
    """(S, ids, scores): S float64 [n, m] with ineligible ids (and the query's
    own, unless keep_self) at -inf, ids int32 [n, k] (-1 where the listed
    score is -inf or k exceeds m), scores float64 [n, k] (-inf there).  rows
    None = every row of T.  `+ 0.0` turns a -0.0 into +0.0, as the library's
    scores never hold -0.0."""
    T64 = np.asarray(T).astype(np.float64)
    m = T64.shape[0]
    rows = np.arange(m) if rows is None else np.asarray(rows, np.int64)
    S = T64[rows] @ T64.T + 0.0
    if cosine:
        nrm = np.sqrt((T64 * T64).sum(axis=1))
        inv = np.divide(1.0, nrm, out=np.zeros_like(nrm), where=nrm > 0)
        S = S * inv[rows][:, None] * inv[None, :] + 0.0
    if mask is not None:
        S[:, np.asarray(mask) == 0] = -np.inf
    if not keep_self:
        S[np.arange(len(rows)), rows] = -np.inf
    ids = np.broadcast_to(np.arange(m), S.shape)
    order = np.lexsort((ids, -S), axis=1)[:, :k]
    sc = np.take_along_axis(S, order, axis=1)
    out = np.where(np.isfinite(sc), order, -1).astype(np.int32)
    if k > m:
        pad = k - m
        out = np.concatenate([out, np.full((len(rows), pad), -1, np.int32)], axis=1)
        sc = np.concatenate([sc, np.full((len(rows), pad), -np.inf)], axis=1)
    return S, out, sc


def grid_table(m, dim, seed):
    """The draw of recommend_ref.grid_inputs' V."""
    return np.random.default_rng(seed).integers(-2, 3, (m, dim)).astype(np.float32)


def sign_table(m, dim, seed, zeros):
    T = (2 * np.random.default_rng(seed).integers(0, 2, (m, dim)) - 1).astype(np.float32)
    if zeros:
        T[0] = 0.0
        T[m - 1] = 0.0
    return T


def gauss_table(m, dim, seed):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((m, dim))
    return (T * 10.0 ** rng.uniform(-1.5, 1.5, (m, 1))).astype(np.float32)


def query_rows(m, n, seed):
    """n query ids of a table of m rows, shuffled: m - 1, 0, 128 and 127 where
    they exist, one of them twice, the rest random (repeats allowed).  A case
    with fewer than five queries keeps the head of that list: n = 1 asks for
    m - 1 alone."""
    need = []
    for r in (m - 1, 0, 128, 127):
        if 0 <= r < m and r not in need:
            need.append(r)
    need.append(need[0])
    rng = np.random.default_rng(seed + 7)
    if n <= len(need):
        return np.array(need[:n], np.int64)
    rows = np.concatenate([need, rng.integers(0, m, n - len(need))]).astype(np.int64)
    rng.shuffle(rows)
    return rows


def dot_main():
    """(m, queries, k kind, dim, mask kind, keep_self, side, splits, seed):
    every table size at every dim, the rest rotated."""
    out = []
    for i, m in enumerate(GRID_M):
        for j, dim in enumerate(GRID_DIMS):
            rows = GRID_ROWS[(i + j) % 4]
            kind = GRID_KINDS[(i + 2 * j) % 3]
            mask = ("none", "m70")[(i // 2 + j) % 2]
            keep = bool((i + j // 2) % 2)
            side = (USER, ITEM)[(i // 3 + j) % 2]
            splits = (None, 1)[(i + j + j // 2) % 2]
            out.append((m, rows, kind, dim, mask, keep, side, splits, 5000 + 10 * i + j))
    return out


def dot_plan():
    """(m, queries, k, dim, mask kind, keep_self, side, splits, seed); splits
    None = the automatic count.  After the rotation the single cases: k above
    the eligible count, nothing eligible, buffers of 512 / 1024 / 2048 slots
    compacted repeatedly by one split, and recommend_ref.CAP_EDGE -- with one
    split and every row eligible the eligible count fills the smallest and
    the largest buffer to its last slot - 1 | 0 | + 1; without keep_self the
    table is one row larger, so that the count is the same."""
    out = [(m, rows, grid_k(m, kind), dim, mask, keep, side, splits, seed)
           for m, rows, kind, dim, mask, keep, side, splits, seed in dot_main()]
    out.append((127, 64, 130, 64, "none", False, ITEM, None, 5901))   # k = m + 3
    out.append((257, 65, 33, 64, "zero", True, USER, None, 5902))     # nothing eligible
    out.append((5000, 65, 33, 5, "none", False, ITEM, 1, 5903))       # 512 slots
    out.append((5000, 65, 200, 5, "none", True, USER, 1, 5904))       # 1024 slots
    out.append((5000, 65, 1024, 64, "m70", False, ITEM, 1, 5905))     # 2048 slots
    for e, (m, k) in enumerate(RR.CAP_EDGE):
        out.append((m, 5, k, 5, "none", True, (USER, ITEM)[e % 2], 1, 5910 + e))
        out.append((m + 1, 5, k, 5, "none", False, (ITEM, USER)[e % 2], 1, 5920 + e))
    return out


def cosine_plan():
    """(m, queries, k, dim, mask kind, keep_self, side, splits, zero rows,
    seed): the sizes, dims, k kinds and query counts of dot_plan() in one
    rotation, every second table with rows 0 and m - 1 all zero."""
    out = []
    for i, m in enumerate(GRID_M):
        dim = GRID_DIMS[i % 4]
        k = grid_k(m, GRID_KINDS[(i + 1) % 3])
        out.append((m, GRID_ROWS[(i + 3) % 4], k, dim, ("none", "m70")[(i // 2) % 2],
                    bool(i % 3 == 0), (ITEM, USER)[i % 2], (None, 1)[(i // 2) % 2], i % 2 == 1,
                    6000 + i))
    out.append((5000, 65, 1024, 64, "none", True, ITEM, 1, True, 6020))   # 2048 slots, zero rows
    out.append((513, 64, 200, 200, "m70", False, USER, None, True, 6021))  # 1024 slots
    return out


def gauss_plan():
    """(m, queries, k, dim, mask kind, keep_self, side, seed)."""
    out = []
    for i, m in enumerate(GAUSS_M):
        for j, dim in enumerate(GAUSS_DIMS):
            out.append((m, 65, GAUSS_KS[(i + j) % 2], dim, ("none", "m70")[(i + j // 2) % 2],
                        (i + j) % 3 == 0, (USER, ITEM)[(i + (j > 0)) % 2], 6100 + 10 * i + j))
    return out


def cosine_tol(Dp):
    """(2 Dp + 8) 2^-24: gamma_Dp for the dot relative to |q||j|, gamma_Dp / 2
    for each of the two norms, and a few roundings for the square root, the
    division and the two multiplies.  Derived, not measured."""
    return (2 * Dp + 8) * 2.0 ** -24


def check_cosine(T, rows, k, keep_self, mask, ids, scores, tol):
    """The conditions on a cosine answer (ids int32 [n, k], scores float32)
    against float64; returns the largest score error.  Every row is checked."""
    S, _, _ = similar64(T, rows, k, True, True, None)   # plain float64 cosines
    m = np.asarray(T).shape[0]
    rows = np.arange(m) if rows is None else np.asarray(rows, np.int64)
    flt_max = np.finfo(np.float32).max
    worst = 0.0
    for i, r in enumerate(rows):
        elig = np.ones(m, bool) if mask is None else np.asarray(mask) != 0
        if not keep_self:
            elig = elig.copy()
            elig[r] = False
        n_list = min(k, int(elig.sum()))
        t = ids[i, :n_list]
        assert (ids[i, n_list:] == -1).all() and (scores[i, n_list:] == -flt_max).all(), i
        assert (t >= 0).all() and len(set(t.tolist())) == n_list and elig[t].all(), i
        sc = scores[i, :n_list].astype(np.float64)
        c64 = S[i, t]
        err = np.abs(sc - c64).max(initial=0.0)
        worst = max(worst, err)
        assert err <= tol, (i, err, tol)
        d = np.diff(sc)
        assert (d <= 0).all(), i
        assert (np.diff(t)[d == 0] > 0).all(), i   # equal scores: ascending id
        if n_list == k:
            rest = elig.copy()
            rest[t] = False
            assert not (S[i, rest] > c64[-1] + 2 * tol).any(), i
        if keep_self and elig[r] and n_list and S[i, r] > 0.5:   # not a zero row
            # its own id is listed with a score within tol of 1, unless k
            # rows that equal it (within the tolerance) fill the list
            assert r in t or c64[-1] >= 1.0 - 2 * tol, i
            if r in t:
                assert abs(float(scores[i, list(t).index(r)]) - 1.0) <= tol, i
    return worst
