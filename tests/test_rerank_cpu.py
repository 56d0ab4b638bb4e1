"""The float64 reference and the case plan of the candidate-ranking tests
(tests/rerank_ref.py), and the surface of the feature, checked without a GPU:
rank64 against a plain Python sort, the pair cover of the plan, the repeats its
lists hold, the Gaussian cases' flagged share in float64 alone, the C entry
points' null-context answer, the Python methods and the header declarations."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import aux_data as A
import rerank_ref as Q
from conftest import ROOT

fh = pytest.importorskip("frecsys_hip")


def _plain(X, V, ptr, col, rows, cp, ci, k, exclude, mask):
    items, scores = [], []
    for i in range(len(cp) - 1):
        r = i if rows is None else rows[i]
        hist = set(int(c) for c in col[ptr[r]:ptr[r + 1]]) if exclude else set()
        cand = []
        for j in sorted(set(int(c) for c in ci[cp[i]:cp[i + 1]])):
            if j in hist or (mask is not None and not mask[j]):
                continue
            s = float(np.dot(X[r].astype(np.float64), V[j].astype(np.float64)))
            cand.append((-s, j))
        cand.sort()
        cand = cand[:k]
        items.append([j for _, j in cand] + [-1] * (k - len(cand)))
        scores.append([-s + 0.0 for s, _ in cand] + [-np.inf] * (k - len(cand)))
    return np.array(items, np.int32), np.array(scores)


def test_rank64_against_plain_sort():
    import recommend_ref as RR
    for n, (m, rows, k, dim, exclude, mk, sub) in enumerate([
            (40, 9, 5, 6, True, "m70", None),
            (40, 9, 50, 6, True, "none", [8, 0, 3, 3]),
            (33, 6, 1, 5, False, "m70", [5, 1])]):
        X, V, ptr, col = RR.grid_inputs(m, rows, k, dim, 60 + n)
        mask = RR.grid_mask(m, mk, 60 + n)
        nl = len(sub) if sub else rows
        cp, ci = Q.grid_lists(m, [0, 1, 7, 90, 12, 30, 2, 5, 64][:nl], 70 + n)
        items, scores = Q.rank64(X, V, ptr, col, sub, cp, ci, k, exclude, mask)
        pi, ps = _plain(X, V, ptr, col, sub, cp, ci, k, exclude, mask)
        np.testing.assert_array_equal(items, pi)
        np.testing.assert_array_equal(scores, ps)
        assert items.shape == (nl, k) and (items[0] == -1).all()   # the empty list


def test_grid_plan_covers_every_pair():
    """Every (length class, k, dim) pair: a main case holds every length, and
    the main cases hold every (k, dim)."""
    main = Q.grid_main()
    assert {(p[2], p[3]) for p in main} == set(itertools.product(Q.GRID_KS, Q.GRID_DIMS))
    for m, rows, k, dim, exclude, mk, shift, seed in main:
        lens = Q.case_lens(rows, k, shift)
        assert set(lens) == {Q.grid_len(L, k) for L in Q.GRID_LENS}, (k, dim)
    for name, idx, want in (("m", 0, Q.GRID_M), ("rows", 1, Q.GRID_ROWS),
                            ("exclude", 4, (False, True)), ("mask", 5, ("none", "m70"))):
        for other, oidx, owant in (("k", 2, Q.GRID_KS),):
            seen = {(p[idx], p[oidx]) for p in main}
            assert seen == set(itertools.product(want, owant)), (name, other)
        assert {p[idx] for p in main} == set(want)
    plan = Q.grid_plan()
    assert plan[:len(main)] == main
    singles = plan[len(main):]
    assert {p[1] for p in singles} >= {1, 65} and any(p[5] == "zero" for p in singles)
    assert {Q.case_lens(p[1], p[2], p[6])[0] for p in singles if p[1] == 1} >= {0, 20000}
    # the kernel's chunk, buffer and cut point, each - 1 | 0 | + 1
    for e in (256, 2048, 1792):
        assert {e - 1, e, e + 1} <= set(Q.GRID_LENS)


def test_grid_lists_hold_repeats_and_ties():
    for case in Q.grid_plan():
        m, rows, k = case[0], case[1], case[2]
        X, V, ptr, col, mask, cp, ci = Q.grid_case(*case)
        assert len(cp) == rows + 1 and ci.min(initial=0) >= 0 and ci.max(initial=0) < m
        for i in range(rows):
            c = ci[cp[i]:cp[i + 1]]
            if len(c) >= 5:
                h = len(c) // 2
                assert c[h] == c[h + 1] == c[h + 2] and c[0] == c[-1]
        if rows >= 33 and case[5] != "zero":
            assert (np.diff(cp) > m).any()    # a list longer than the catalogue
            items, sc = Q.rank64(X, V, ptr, col, None, cp, ci, k, case[4], mask)
            fin = np.isfinite(sc[:, :-1]) & np.isfinite(sc[:, 1:]) if k > 1 else np.zeros(0, bool)
            assert k == 1 or (fin & (sc[:, :-1] == sc[:, 1:])).any(), case   # exact ties listed
            assert (items == -1).any() or k == 1   # short lists leave empty slots


def test_gauss_seeds_keep_float64_under_the_flag_limit():
    assert {c for c, _ in Q.GAUSS_CASES} <= set(A.topk_cases())
    assert {c[0] for c, _ in Q.GAUSS_CASES} == set(A.TOPK_M)
    for (m, rows, k, dim, seed), ls in Q.GAUSS_CASES:
        Ue, V, ep, ec, S, _, _ = A.topk_inputs(m, rows, k, dim, seed)
        fin = np.isfinite(S)
        tol = 2e-6 * np.abs(S[fin]).max()
        cp, ci = Q.gauss_lists(m, rows, ls)
        _, sc = Q.rank64(Ue, V, ep, ec, None, cp, ci, k + 1, True, None)
        assert Q.gauss_flagged(sc, tol).sum() <= 0.05 * rows, (m, rows, k, dim)


def test_entry_points_reject_a_null_context():
    lib = fh.load_library()
    one64 = np.zeros(2, np.int64)
    one32 = np.zeros(2, np.int32)
    out = np.zeros(2, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.frecsys_score_pairs(None, fh.SIDE_USER, P(one64), P(one32), 1, P(out)) == fh.ERR_INVALID
    assert lib.frecsys_rank_candidates(None, fh.SIDE_USER, None, 1, P(one64), P(one32), 1, 0, None,
                                       P(one32), P(out)) == fh.ERR_INVALID
    ml = fh.load_model_library()
    assert ml.frecsys_model_score(None, P(one64), P(one32), 1, P(out)) == fh.ERR_INVALID
    assert ml.frecsys_model_rank_candidates(None, P(one64), 1, P(one64), P(one32), 1, 0, None,
                                            P(one32), P(out)) == fh.ERR_INVALID
    assert ml.frecsys_model_rank_candidates_fold_in(None, P(one64), P(one32), 1, P(one64), P(one32),
                                                    1, 0, None, P(one32), P(out)) == fh.ERR_INVALID


def test_python_surface():
    for name in ("score_pairs", "rank_candidates"):
        assert callable(getattr(fh.Context, name))
    for name in ("score", "rank_candidates", "rank_candidates_fold_in"):
        assert callable(getattr(fh.Model, name))
    assert {"frecsys_score_pairs", "frecsys_rank_candidates"} <= set(fh.EXPORTS)
    assert {"frecsys_model_score", "frecsys_model_rank_candidates",
            "frecsys_model_rank_candidates_fold_in"} <= set(fh.MODEL_EXPORTS)


def test_headers_declare_the_entry_points():
    def decls(path):
        txt = open(os.path.join(ROOT, "include", path)).read()
        return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    core, model = decls("frecsys_hip.h"), decls("frecsys_model.h")
    assert re.search(r"int frecsys_score_pairs\(frecsys_ctx\*[^;]*const int64_t\* rows,\s*"
                     r"const int32_t\* items,\s*int64_t n_pairs,\s*float\* scores\);", core)
    assert re.search(r"int frecsys_rank_candidates\(frecsys_ctx\*[^;]*const int64_t\* cand_ptr,\s*"
                     r"const int32_t\* cand_items,\s*int32_t k,\s*int32_t flags,[^;]*\);", core)
    for name in ("frecsys_model_score", "frecsys_model_rank_candidates",
                 "frecsys_model_rank_candidates_fold_in"):
        assert re.search(r"int %s\(frecsys_model\* m," % name, model), name
