"""The float64 reference and the integer-grid cases of the recommend tests
(tests/recommend_ref.py), checked without a GPU: recommend64 against a plain
Python sort, the pair cover of the case plan, and that the cases do hold the
exact ties they are there for."""
import itertools

import numpy as np

import recommend_ref as RR


def _plain(X, V, ptr, col, rows, k, exclude, mask):
    """The ranking by a Python sort of (score, id) tuples."""
    items, scores = [], []
    rows = range(len(X)) if rows is None else rows
    for r in rows:
        hist = set(int(c) for c in col[ptr[r]:ptr[r + 1]]) if exclude else set()
        cand = []
        for j in range(len(V)):
            if j in hist or (mask is not None and not mask[j]):
                continue
            s = float(np.dot(X[r].astype(np.float64), V[j].astype(np.float64)))
            cand.append((-s, j))
        cand.sort()
        cand = cand[:k]
        items.append([j for _, j in cand] + [-1] * (k - len(cand)))
        scores.append([-s for s, _ in cand] + [-np.inf] * (k - len(cand)))
    return np.array(items, np.int32), np.array(scores)


def test_recommend64_against_plain_sort():
    cases = [
        (7, 5, 3, 4, True, "none", None),
        (40, 9, 50, 6, True, "m70", [8, 0, 3, 3]),   # k past the item count, repeated rows
        (33, 6, 33, 5, False, "m70", [5, 1]),
    ]
    for n, (m, rows, k, dim, exclude, mk, sub) in enumerate(cases):
        X, V, ptr, col = RR.grid_inputs(m, rows, k, dim, 50 + n)
        mask = RR.grid_mask(m, mk, 50 + n)
        _, items, scores = RR.recommend64(X, V, ptr, col, sub, k, exclude, mask)
        pi, ps = _plain(X, V, ptr, col, sub, k, exclude, mask)
        np.testing.assert_array_equal(items, pi)
        np.testing.assert_array_equal(scores, ps)
        assert items.shape == (len(sub) if sub else rows, k)


def test_grid_plan_covers_every_pair():
    main = RR.grid_main()
    names = ("m", "rows", "kind", "dim", "exclude", "mask")
    cols = {nm: [p[i] for p in main] for i, nm in enumerate(names)}
    want = {"m": RR.GRID_M, "rows": RR.GRID_ROWS, "kind": RR.GRID_KINDS, "dim": RR.GRID_DIMS,
            "exclude": (False, True), "mask": ("none", "m70")}
    for a, b in itertools.combinations(names, 2):
        seen = set(zip(cols[a], cols[b]))
        missing = [(x, y) for x in want[a] for y in want[b] if (x, y) not in seen]
        assert not missing, (a, b, missing)
    singles = RR.grid_plan()[len(main):]
    assert RR.grid_plan()[:len(main)] == [
        (m, rows, RR.grid_k(m, kind), dim, ex, mk, None, seed)
        for m, rows, kind, dim, ex, mk, seed in main]
    assert any(p[2] == p[0] + 3 and 8 <= p[0] <= 1021 for p in singles)
    assert any(p[5] == "zero" for p in singles)
    assert {(p[0], p[2]) for p in singles if p[6] == 1} >= set(RR.CAP_EDGE) | {(5000, 33)}


def test_grid_cases_hold_exact_ties():
    """Every case with more than one item has two equal eligible scores inside
    a list; a list of one (k = 1) cannot, so such a case has two equal
    eligible scores in a row instead (what the running threshold of a k = 1
    sweep meets).  At least one case has a tie straddling the k-th place of a
    list that also ties inside."""
    straddle_and_inside = 0
    for m, rows, k, dim, exclude, mk, _, seed in RR.grid_plan():
        if m == 1 or mk == "zero":
            continue
        X, V, ptr, col = RR.grid_inputs(m, rows, k, dim, seed)
        S, items, sc = RR.recommend64(X, V, ptr, col, None, k, exclude, RR.grid_mask(m, mk, seed))
        full = -np.sort(-S, axis=1)
        with np.errstate(invalid="ignore"):
            tie = np.isfinite(full[:, :-1]) & (full[:, :-1] == full[:, 1:])
        inside = tie[:, :k - 1].any() if k >= 2 else False
        at_kth = tie[:, k - 1].any() if tie.shape[1] >= k else False
        assert inside or (k == 1 and tie.any()), (m, rows, k, dim)
        straddle_and_inside += bool(inside and at_kth)
    assert straddle_and_inside >= 1
