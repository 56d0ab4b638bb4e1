"""Float64 reference, inputs and case plans for the DPP calls
(frecsys_dpp_select, frecsys_diversify_dpp, frecsys_recommend_dpp; helper of
tests/test_dpp_cpu.py, tests/test_dpp_gpu.py and tests/test_dpp_model_gpu.py;
not a test).

dpp64()        the greedy selection of include/frecsys_hip.h in float64 with
               the true exp2, per row: the selected slots, their gains, and the
               first step that is `close` (k when none is): its best value is
               within `tol` (relative) of the runner-up, or some unselected
               residual lies within 1 % of eps -- from there on a float32
               selection may rightly differ.
kernel64()     L = diag(sqrt w) S diag(sqrt w) of one row's filled slots in
               float64: what the brute-force and log-det tests take
               determinants of.
factor_in_lds()  the kernel's rule for where the factor C lives (kDppLdsBytes
               of csrc/kernels.h, mirrored here).
gpu_plan()     the rotated cases of the byte-for-byte GPU test, with (pool, k)
               pairs on both sides of that switch.
The input makers are tests/diverse_ref.py's: top_pools, gauss_case,
random_pools, item_table.
"""
import numpy as np

import diverse_ref as D

FLT_MAX = D.FLT_MAX
top_pools, gauss_case, gauss_table = D.top_pools, D.gauss_case, D.gauss_table
random_pools, item_table = D.random_pools, D.item_table

POOLS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024)
DIMS = (5, 64, 200, 500, 1000)
ROWS = (1, 63, 65)
CATALOGUES = (129, 5000)
THETAS = (0.0, 2.0, 8.0)
K_KINDS = ("one", "all", "third")
DPP_LDS_BYTES = 40 * 1024  # kDppLdsBytes


def factor_in_lds(pool, k):
    return 4 * k * pool <= DPP_LDS_BYTES


def _row(T64, ids_row, sc_row, theta, raw):
    """(filled slots, unit rows, w float64) of one pool row."""
    filled = np.flatnonzero(ids_row >= 0)
    rows = T64[ids_row[filled]]
    sc = np.asarray(sc_row[filled], np.float64)
    if raw:
        rel = sc
    else:
        rng = sc.max() - sc.min() if len(sc) else 0.0
        rel = (sc - sc.min()) / rng if rng > 0 else np.zeros_like(sc)
    nrm = np.sqrt((rows * rows).sum(1))
    inv = np.divide(1.0, nrm, out=np.zeros_like(nrm), where=nrm > 0)
    w = np.exp2(np.clip(theta * rel, -64.0, 64.0))
    return filled, rows * inv[:, None], w


def kernel64(T, ids_row, sc_row, theta, raw):
    """(filled slots, L float64 [p, p])."""
    filled, U, w = _row(np.asarray(T, np.float64), np.asarray(ids_row), sc_row, theta, raw)
    q = np.sqrt(w)
    return filled, (U @ U.T) * q[:, None] * q[None, :]


def dpp64(T, ids, scores, k, theta, eps, raw, tol=1e-4):
    """(slots int [n, k] (-1 beyond the filled count), gains float64 [n, k]
    (0 in the fallback, -inf beyond the filled count), first close step int
    [n])."""
    T64 = np.asarray(T, np.float64)
    ids = np.asarray(ids)
    n, P = ids.shape
    slots = np.full((n, k), -1, np.int64)
    gains = np.full((n, k), -np.inf)
    flag = np.full(n, k, np.int64)
    for i in range(n):
        filled, U, w = _row(T64, ids[i], scores[i], theta, raw)
        p = len(filled)
        if p == 0:
            continue
        S = U @ U.T
        r = ((U * U).sum(1) > 0).astype(np.float64)
        alive = np.ones(p, bool)
        C = np.zeros((0, p))
        for t in range(min(k, p)):
            if flag[i] == k and (np.abs(r[alive] - eps) <= 0.01 * eps).any():
                flag[i] = t
            E = alive & (r >= eps)
            if not E.any():
                s = int(np.flatnonzero(alive)[0])
                slots[i, t], gains[i, t] = filled[s], 0.0
                alive[s] = False
                continue
            v = np.where(E, w * r, -np.inf)
            s = int(np.argmax(v))  # the first of equal values: the lower slot
            rest = v.copy()
            rest[s] = -np.inf
            if flag[i] == k and E.sum() > 1 and v[s] - rest.max() <= tol * v[s]:
                flag[i] = t
            slots[i, t], gains[i, t] = filled[s], v[s]
            alive[s] = False
            e = (S[s] - C.T @ C[:, s]) / np.sqrt(r[s])
            e[~alive] = 0.0
            C = np.vstack([C, e])
            r = r - e * e
    return slots, gains, flag


def plan_k(pool, kind):
    return {"one": 1, "all": pool, "third": -(-pool // 3)}[kind]


# (pool, k) straddling 4 k pool = DPP_LDS_BYTES: the last shape in LDS and the
# first in the workspace, at a pool on a lane seam and at one off it
SWITCH = ((128, 80), (128, 81), (257, 39), (257, 40))


def gpu_plan():
    """(pool, k, dim, rows, items, theta, raw, grid, seed): every pool size once
    per k kind and the SWITCH pairs, the other parameters rotated so that every
    dim, row count, catalogue, theta, mode and table kind occurs with small and
    large pools.  The host reference costs rows * pool * k * (dim + k / 2) at
    the most: the largest pools run few rows when k is large."""
    shapes = [(pool, plan_k(pool, kind)) for pool in POOLS for kind in K_KINDS]
    shapes = list(dict.fromkeys(shapes)) + list(SWITCH)
    out = []
    for q, (pool, k) in enumerate(shapes):
        i, j = q // 3, q % 3
        dim = DIMS[(i + 2 * j) % 5]
        rows = ROWS[(i + j) % 3]
        cost = pool * k * (dim + k / 2)
        if cost * rows > 2e9:
            rows = 1 if cost * 63 > 2e9 else 63
        out.append((pool, k, dim, rows, CATALOGUES[(i + j) % 2], THETAS[(i // 2 + j) % 3],
                    bool((i + j // 2) % 2), bool((i // 3 + j) % 2), 9000 + 10 * i + j))
    assert any(factor_in_lds(p, k) and k > 1 for p, k, *_ in out)
    assert any(not factor_in_lds(p, k) for p, k, *_ in out)
    return out
