"""Float64 reference, float32 mirror, inputs and case plans for the MMR calls
(frecsys_mmr_select, frecsys_diversify, frecsys_recommend_diverse; helper of
tests/test_diverse_cpu.py, tests/test_diverse_gpu.py and
tests/test_diverse_model_gpu.py; not a test).

mmr64()        the greedy selection of include/frecsys_hip.h in float64, per
               row: the selected slots, their values, and the first step whose
               best value is less than `tol` above the second best (k when no
               step is that close) -- from there on a float32 selection may
               rightly differ.
mmr32()        the same steps in numpy float32, operation by operation; the
               dot products are taken in float64 and rounded once, so it is the
               library's chain only where every dot is exact in float32 (the
               sign and grid tables below).
top_pools()    pools as frecsys_recommend leaves them: the `pool` best items of
               each query by (score descending, id ascending), float32 scores.
exact_case()   sign table x grid queries: every quantity of the raw-score mode
               is an exact dyadic float32.
gauss_case()   Gaussian tables with rows scaled over two decades.
random_pools() pools "from anywhere": random ids with repeats, empty slots in
               the middle and at the tail, optionally a zero item row and rows
               with fewer filled slots than k.
gpu_plan()     the rotated cases of the byte-for-byte GPU test.
"""
import numpy as np

import recommend_ref as RR
import similar_ref as SR

FLT_MAX = np.finfo(np.float32).max

POOLS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024)
DIMS = (5, 64, 200, 500, 1000)
ROWS = (1, 63, 65)
CATALOGUES = (129, 5000)
LAMS = (0.0, 0.5, 1.0)
K_KINDS = ("one", "all", "third")


def plan_k(pool, kind):
    return {"one": 1, "all": pool, "third": -(-pool // 3)}[kind]


def mmr64(T, ids, scores, k, lam, raw, tol):
    """(slots int [n, k] (-1 beyond the filled count), values float64 [n, k],
    first close step int [n])."""
    T64 = np.asarray(T, np.float64)
    ids = np.asarray(ids)
    n, P = ids.shape
    slots = np.full((n, k), -1, np.int64)
    vals = np.full((n, k), -np.inf)
    flag = np.full(n, k, np.int64)
    for i in range(n):
        filled = np.flatnonzero(ids[i] >= 0)
        if len(filled) == 0:
            continue
        rows = T64[ids[i, filled]]
        sc = np.asarray(scores[i, filled], np.float64)
        if raw:
            rel = sc
        else:
            rng = sc.max() - sc.min()
            rel = (sc - sc.min()) / rng if rng > 0 else np.zeros_like(sc)
        nrm = np.sqrt((rows * rows).sum(1))
        inv = np.divide(1.0, nrm, out=np.zeros_like(nrm), where=nrm > 0)
        U = rows * inv[:, None]
        base = lam * rel
        m = np.full(len(filled), -np.inf)
        alive = np.ones(len(filled), bool)
        for t in range(min(k, len(filled))):
            v = base + 0.0 if t == 0 else (base - (1.0 - lam) * m) + 0.0
            v = np.where(alive, v, -np.inf)
            s = int(np.argmax(v))  # the first of equal values: the lower slot
            rest = v.copy()
            rest[s] = -np.inf
            if flag[i] == k and alive.sum() > 1 and v[s] - rest.max() < tol:
                flag[i] = t
            slots[i, t] = filled[s]
            vals[i, t] = v[s]
            alive[s] = False
            m = np.maximum(m, U @ U[s] + 0.0)
    return slots, vals, flag


def mmr32(T, ids, scores, k, lam, raw):
    """(items int32 [n, k], scores float32 [n, k], mmr float32 [n, k]) by the
    steps of frecsys_mmr_select in numpy float32."""
    f = np.float32
    T64 = np.asarray(T, np.float64)
    ids = np.asarray(ids, np.int32)
    scores = np.asarray(scores, np.float32)
    n, P = ids.shape
    out_i = np.full((n, k), -1, np.int32)
    out_s = np.full((n, k), -FLT_MAX, np.float32)
    out_m = np.full((n, k), -FLT_MAX, np.float32)
    lam, zero = f(lam), f(0.0)
    oml = f(1.0) - lam
    for i in range(n):
        filled = np.flatnonzero(ids[i] >= 0)
        if len(filled) == 0:
            continue
        rows = T64[ids[i, filled]]
        sc = scores[i, filled]
        if raw:
            rel = sc
        else:
            smax, smin = sc.max(), sc.min()
            rng = smax - smin
            rel = (sc - smin) / rng if rng > 0 else np.zeros_like(sc)
        n2 = (rows * rows).sum(1).astype(f)
        with np.errstate(divide="ignore"):
            inv = np.where(n2 > 0, f(1.0) / np.sqrt(n2), zero).astype(f)
        base = (lam * rel).astype(f)
        m = np.full(len(filled), -np.inf, f)
        alive = np.ones(len(filled), bool)
        for t in range(min(k, len(filled))):
            v = base + zero if t == 0 else (base - oml * m) + zero
            v = np.where(alive, v, -np.inf).astype(f)
            s = int(np.argmax(v))
            out_i[i, t] = ids[i, filled[s]]
            out_s[i, t] = sc[s]
            out_m[i, t] = v[s]
            alive[s] = False
            g = (rows @ rows[s]).astype(f)
            m = np.maximum(m, ((g * inv[s]) * inv + zero).astype(f))
    return out_i, out_s, out_m


def top_pools(X, V, pool):
    """(ids int32 [n, pool], scores float32 [n, pool]): recommend64's lists
    with float32 scores (exact for the grid and sign tables), -1 / -FLT_MAX
    beyond the item count."""
    _, items, sc = RR.recommend64(X, V, None, None, None, pool, False, None)
    scores = np.where(items >= 0, sc, -FLT_MAX).astype(np.float32)
    return items.astype(np.int32), scores


def exact_case(dim, n, m, pool, seed):
    """(T, ids, scores): a sign table (every inverse norm the same power of
    two at dim 16 / 64 / 256) and the pools of integer-grid queries."""
    T = SR.sign_table(m, dim, seed, zeros=False)
    X = RR.grid_inputs(m, n, pool, dim, seed + 1)[0]
    ids, scores = top_pools(X, T, pool)
    return T, ids, scores


def gauss_table(m, dim, seed):
    """Gaussian rows, each scaled by 10^u with u uniform in [-1, 1]."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((m, dim))
    return (T * 10.0 ** rng.uniform(-1.0, 1.0, (m, 1))).astype(np.float32)


def gauss_case(dim, n, m, pool, seed):
    T = gauss_table(m, dim, seed)
    X = np.random.default_rng(seed + 1).standard_normal((n, dim)).astype(np.float32)
    ids, scores = top_pools(X, T, pool)
    return T, ids, scores


def random_pools(n, m, pool, k, seed, grid):
    """(ids, scores) from anywhere: ids uniform in [0, m) with repeats, scores
    Gaussian (grid: small integers, heavy ties), about one slot in eight empty
    -- the last slots of row 0 among them --, item 0 in some slot of every
    second row, and every fifth row with fewer than k filled slots (when k >
    1)."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, m, (n, pool)).astype(np.int32)
    if grid:
        scores = rng.integers(-3, 4, (n, pool)).astype(np.float32)
    else:
        scores = rng.standard_normal((n, pool)).astype(np.float32)
    ids[::2, rng.integers(0, pool)] = 0
    ids[rng.random((n, pool)) < 0.125] = -1
    ids[0, pool - (pool // 4):] = -1
    if k > 1:
        for i in range(0, n, 5):
            keep = rng.permutation(pool)[: k - 1 - (i % 2)]
            row = np.full(pool, -1, np.int32)
            row[keep] = ids[i, keep]
            ids[i] = row
    return ids, scores


def item_table(m, dim, seed, grid):
    """The item table of a GPU case; row 0 is all zero."""
    T = SR.grid_table(m, dim, seed) if grid else gauss_table(m, dim, seed)
    T[0] = 0.0
    return T


def gpu_plan():
    """(pool, k, dim, rows, items, lam, raw, grid, seed): every pool size once
    per k kind, the other parameters rotated so that every dim, row count,
    catalogue, lam, mode and table kind occurs with small and large pools.
    The host reference costs rows * pool * k * dim: the largest pools run few
    rows or a small dim when k = pool."""
    out = []
    for i, pool in enumerate(POOLS):
        for j, kind in enumerate(K_KINDS):
            k = plan_k(pool, kind)
            dim = DIMS[(i + 2 * j) % 5]
            rows = ROWS[(i + j) % 3]
            if pool * k * dim * rows > 3e9:
                rows = 1 if pool * k * dim * 63 > 3e9 else 63
            out.append((pool, k, dim, rows, CATALOGUES[(i + j) % 2], LAMS[(i // 2 + j) % 3],
                        bool((i + j // 2) % 2), bool((i // 3 + j) % 2), 8000 + 10 * i + j))
    return out
