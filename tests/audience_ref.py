"""Float64 reference and exact inputs for frecsys_audience (helper of
tests/test_audience_cpu.py, tests/test_audience_gpu.py and
tests/test_audience_model_gpu.py; not a test).

audience64()    recommend_ref.recommend64 with the roles swapped: the item rows
                are the queries, the users the table searched, the ITEM-side
                CSR the histories; float64 scores, `+ 0.0`, the k first by
                (score descending, user id ascending).
grid_case()     the inputs of one exact case: integer-grid tables of {-2..2}
                (recommend_ref.grid_inputs: every score an exact integer, heavy
                ties), aux_data.aux_eval's rows as the ITEM CSR, a query id
                repeated inside the first pass, one all-zero query and one
                all-zero user row.
grid_plan()     the cases of the exact GPU tests, every kernel seam taken from
                a plan function (fh.audience_plan): C = chunk_rows, QT =
                queries_per_pass, the slot counts of the smallest and the
                largest buffer.
"""
import numpy as np

import recommend_ref as RR

GRID_DIMS = (5, 20, 64, 200, 500, 1000)
GRID_KINDS = ("one", "k33", "max", "over")  # k = 1, 33, min(m, 1024), m + 3
GRID_MASKS = ("none", "m70", "zero")
GRID_CASES = 7 * 6 + 6 + 3   # len(grid_plan()): the rotated part, the capacity edges, the sweeps


def audience64(V, U, iptr, icol, items, k, exclude, mask):
    """(S, users, scores): S float64 [n, m] with ineligible users at -inf,
    users int32 [n, k] (-1 where nothing eligible is left), scores float64
    [n, k].  V: item table (queries), U: user table, iptr / icol: the ITEM-side
    CSR (users per item), items: query ids or None = every item."""
    return RR.recommend64(V, U, iptr, icol, items, k, exclude, mask)


def grid_k(m, kind):
    return {"one": 1, "k33": 33, "max": min(m, 1024), "over": min(m + 3, 1024)}[kind]


def grid_sizes(plan_fn):
    """(C, QT, users m, queries n) of the grid: the sizes around one chunk of
    the table and one pass of queries."""
    p = plan_fn(64, 5000, 1, 33)
    C, QT = p["chunk_rows"], p["queries_per_pass"]
    return C, QT, (1, 2, C - 1, C, C + 1, 2 * C + 1, 5000), (1, 2, QT - 1, QT, QT + 1, 2 * QT + 1)


def grid_main(plan_fn):
    """(m, n, k kind, dim, exclude, mask kind, seed): every user count at every
    dim; queries, k kind, mask and exclusion rotated so that every pair of
    values of two parameters occurs (test_audience_cpu checks the cover)."""
    _, _, ms, ns = grid_sizes(plan_fn)
    out = []
    for i, m in enumerate(ms):
        for j, dim in enumerate(GRID_DIMS):
            n = ns[(i + j) % 6]
            kind = GRID_KINDS[(i + 2 * j + j // 2) % 4]
            mask = GRID_MASKS[(i + 2 * j + j // 3) % 3]
            exclude = bool((j + i // 2) % 2)
            out.append((m, n, kind, dim, exclude, mask, 7000 + 10 * i + j))
    return out


def grid_plan(plan_fn):
    """(m, n, k, dim, exclude, mask kind, splits, seed); splits None = the
    automatic count.  After the rotated part, with one split (one workgroup
    sees every user, every user eligible, no threshold before the first
    compaction): user counts of slots - 1 | slots | slots + 1 for the smallest
    (k = 33) and the largest (k = 1024) buffer, and 5,000 users through each
    buffer size, compacted more than once."""
    out = [(m, n, grid_k(m, kind), dim, exclude, mask, None, seed)
           for m, n, kind, dim, exclude, mask, seed in grid_main(plan_fn)]
    seed = 7900
    for k in (33, 1024):
        slots = plan_fn(5, 5000, 5, k)["slots"]
        for m in (slots - 1, slots, slots + 1):
            out.append((m, 5, k, 5, False, "none", 1, seed))
            seed += 1
    out.append((5000, 9, 33, 20, True, "none", 1, 7910))
    out.append((5000, 9, 200, 20, False, "none", 1, 7911))
    out.append((5000, 9, 1024, 64, False, "m70", 1, 7912))
    return out


def grid_case(m, n, k, dim, seed):
    """(V, U, iptr, icol, items): n + 1 item rows and m user rows of {-2..2};
    iptr / icol: aux_data.aux_eval over the item rows (row 0 empty, row 1
    {0, m - 1}, row 2 with repeated ids, row 3 leaving k - 1 users free);
    items: 0 .. n-1, with item 1 again in slot 4 (inside the first pass) when
    n >= 5; item 5 is all zero when n >= 6, user m // 2 when m >= 2."""
    V, U, iptr, icol = RR.grid_inputs(m, n + 1, k, dim, seed)
    V = V.copy()
    U = U.copy()
    items = np.arange(n, dtype=np.int64)
    if n >= 5:
        items[4] = 1
    if n >= 6:
        V[5] = 0.0
    if m >= 2:
        U[m // 2] = 0.0
    return V, U, iptr, icol, items
