"""The host half of the evaluate API, no GPU needed: frecsys_list_metrics
(the reference's RankMetrics) and frecsys_metric_cvar (EvaluationResult::cvar)
of libfrecsys_hip.so, and the names the new layers export.

test_list_metrics_equals_oracle   bitwise equal to the CPU oracle's
                                  oracle_evaluate on integer-grid tables
                                  (exact scores, heavy ties), the lists from
                                  the float64 reference recommend64.
test_minus_one_is_never_a_hit     hand-written rows.
test_metric_cvar_equals_reference bitwise equal to metrics_ref.cvar_ref, the
                                  zeros of the quirks asserted.
test_bad_arguments                FRECSYS_ERR_INVALID.
test_names_exported               headers, EXPORTS / MODEL_EXPORTS, methods.
"""
import os

import numpy as np
import pytest

import frecsys_hip as fh
import metrics_ref as MR
import oracle as O
import recommend_ref as RR
from conftest import ROOT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("m,rows,k_list,seed", MR.grid_cases())
def test_list_metrics_equals_oracle(m, rows, k_list, seed):
    K = max(k_list)
    X, V, ptr, col = RR.grid_inputs(m, rows, K, MR.GRID_DIM, seed)
    _, lists, _ = RR.recommend64(X, V, ptr, col, None, K, True, None)
    assert lists.shape == (rows, K)
    gp, gi = MR.ground_truth(rows, m, ptr, col, seed + 5, kmax=min(K, 128))
    for i in range(rows):  # disjoint, so the oracle's -FLT_MAX entries cannot be hits
        h, g = set(col[ptr[i]:ptr[i + 1]].tolist()), set(gi[gp[i]:gp[i + 1]].tolist())
        assert not (h & g) or len(h) == m
    rec, ndcg = fh.list_metrics(lists, gp, gi, k_list)
    orec, ondcg = O.evaluate(X, V, ptr, col, gp, gi, k_list)
    r64, n64 = MR.metrics64(lists, gp, gi, k_list)
    assert np.array_equal(_bits(rec), _bits(orec)), (rec - r64, orec - r64)
    assert np.array_equal(_bits(ndcg), _bits(ondcg)), (ndcg - n64, ondcg - n64)
    assert rec.max() > 0 or rows == 1 or K == 1   # the cases are not all misses
    if K > m:
        assert (lists[:, m:] == -1).all()


def test_minus_one_is_never_a_hit():
    k_list = (1, 3, 4)
    lists = np.array([[-1, -1, -1, -1],
                      [7, 8, 9, 2],
                      [5, 6, 1, 0]], np.int32)
    #  row 0: nothing listed; row 1: the only hit at the last rank; row 2: the
    #  ground truth {5, 1, 9} given as 5 1 5 9 1 -- g counts distinct ids
    gt = [[3], [2], [5, 1, 5, 9, 1]]
    gp = np.concatenate([[0], np.cumsum([len(g) for g in gt])]).astype(np.int64)
    gi = np.concatenate(gt).astype(np.int32)
    rec, ndcg = fh.list_metrics(lists, gp, gi, k_list)
    r64, n64 = MR.metrics64(lists, gp, gi, k_list)
    assert (rec[0] == 0).all() and (ndcg[0] == 0).all()
    np.testing.assert_array_equal(rec[1], np.float32([0, 0, 1]))
    # one hit at rank 3 against an ideal hit at rank 0: 1 / log2(5)
    np.testing.assert_array_equal(ndcg[1], np.float32([0, 0, 1.0 / np.log2(5.0)]))
    # g = 3: recall@1 = 1/1, @3 = 2/3, @4 = 2/3
    np.testing.assert_array_equal(rec[2], np.float32([1.0, 2.0 / 3.0, 2.0 / 3.0]))
    # both are double computations rounded to fp32 once: at most one fp32 ulp apart
    assert (np.abs(rec - r64) <= np.spacing(np.float32(1.0))).all()
    assert (np.abs(ndcg - n64) <= np.spacing(np.float32(1.0))).all()
    assert ndcg[2, 0] == 1.0 and 0 < ndcg[2, 1] < 1


ALPHAS = (MR.DEFAULT_ALPHAS, (0.0,), (1.0,), (0.3, 0.3), (0.5, 0.1))


@pytest.mark.parametrize("n", [1, 7, 10, 1000])
def test_metric_cvar_equals_reference(n):
    v = np.random.default_rng(900 + n).random(n).astype(np.float32)
    for alphas in ALPHAS:
        got = fh.metric_cvar(v, alphas)
        ref = MR.cvar_ref(v, alphas)
        assert got.dtype == np.float32 and got.shape == (len(alphas),)
        assert np.array_equal(_bits(got), _bits(ref)), (n, alphas, got, ref)
    # alpha = 1: position n is never reached, the slot stays 0
    assert fh.metric_cvar(v, (1.0,))[0] == 0.0
    # alpha = 0: the smallest value alone
    assert fh.metric_cvar(v, (0.0,))[0] == v.min()
    # (0.5, 0.1): 0.1's position comes first and its result goes to slot 0
    # (match order); the scan then starts at j = 1 and never looks at 0.5
    # again: slot 1 stays 0
    got = fh.metric_cvar(v, (0.5, 0.1))
    if n > 1:
        assert got[0] != 0.0 and got[1] == 0.0
        assert got[0] == fh.metric_cvar(v, (0.1,))[0]
    # (0.3, 0.3): both match at the same position, in one scan
    got = fh.metric_cvar(v, (0.3, 0.3))
    assert got[0] == got[1] != 0.0


def test_bad_arguments():
    lib = fh.load_library()
    P = fh._ptr
    lists = np.zeros((2, 8), np.int32)
    rec = np.zeros((2, 2), np.float32)
    ndcg = np.zeros((2, 2), np.float32)

    def call(gp, gi, ks, nk=None, list_k=8, lists_=lists, rec_=rec, ndcg_=ndcg):
        gp = np.asarray(gp, np.int64)
        gi = np.asarray(gi, np.int32)
        ks = np.asarray(ks, np.int32)
        return lib.frecsys_list_metrics(P(lists_), 2, list_k, P(gp), P(gi), P(ks),
                                        len(ks) if nk is None else nk, P(rec_), P(ndcg_))

    assert call([0, 1, 3], [1, 2, 3], [2, 8]) == fh.OK
    assert call([0, 0, 3], [1, 2, 3], [2, 8]) == fh.ERR_INVALID      # empty ground-truth row
    assert call([0, 3, 3], [1, 2, 3], [2, 8]) == fh.ERR_INVALID
    assert call([1, 2, 3], [1, 2, 3], [2, 8]) == fh.ERR_INVALID      # gt_ptr[0] != 0
    assert call([0, 2, 1], [1, 2, 3], [2, 8]) == fh.ERR_INVALID      # not monotone
    assert call([0, 1, 3], [1, 2, 3], [2, 8], nk=0) == fh.ERR_INVALID
    assert call([0, 1, 3], [1, 2, 3], [1] * 33, rec_=np.zeros((2, 33), np.float32),
                ndcg_=np.zeros((2, 33), np.float32)) == fh.ERR_INVALID
    assert call([0, 1, 3], [1, 2, 3], [1] * 32, rec_=np.zeros((2, 32), np.float32),
                ndcg_=np.zeros((2, 32), np.float32)) == fh.OK
    assert call([0, 1, 3], [1, 2, 3], [0, 8]) == fh.ERR_INVALID      # k = 0
    assert call([0, 1, 3], [1, 2, 3], [2, 1025], list_k=8) == fh.ERR_INVALID
    assert call([0, 1, 3], [1, 2, 3], [2, 9]) == fh.ERR_INVALID      # list_k < max k
    assert call([0, 1, 3], [1, -2, 3], [2, 8]) == fh.ERR_INVALID     # negative id
    assert call([0, 1, 3], [1, 2, 3], [2, 8], rec_=None) == fh.ERR_INVALID
    assert call([0, 1, 3], [1, 2, 3], [2, 8], ndcg_=None) == fh.ERR_INVALID
    assert call([0, 1, 3], [1, 2, 3], [2, 8], lists_=None) == fh.ERR_INVALID
    assert b"list_metrics" in lib.frecsys_last_error(None)
    with pytest.raises(fh.FrecsysError) as ei:
        fh.list_metrics(lists, [0, 0, 1], [1], (2,))
    assert ei.value.code == fh.ERR_INVALID
    v = np.ones(3, np.float32)
    assert lib.frecsys_metric_cvar(P(v), 3, None, 1, P(v)) == fh.ERR_INVALID
    assert lib.frecsys_metric_cvar(None, 3, P(v), 1, P(v)) == fh.ERR_INVALID
    assert lib.frecsys_metric_cvar(P(v), 3, P(v), 1, None) == fh.ERR_INVALID
    assert lib.frecsys_metric_cvar(P(v), -1, P(v), 1, P(v)) == fh.ERR_INVALID


def test_names_exported():
    hip = open(os.path.join(ROOT, "include", "frecsys_hip.h")).read()
    model = open(os.path.join(ROOT, "include", "frecsys_model.h")).read()
    for name in ("frecsys_list_metrics", "frecsys_metric_cvar", "frecsys_rank_metrics"):
        assert name + "(" in hip and name in fh.EXPORTS
        assert getattr(fh.load_library(), name) is not None
    for name in ("frecsys_model_evaluate", "frecsys_model_evaluate_fold_in"):
        assert name + "(" in model and name in fh.MODEL_EXPORTS
        assert getattr(fh.load_model_library(), name) is not None
    assert callable(fh.Context.rank_metrics)
    assert callable(fh.Model.evaluate) and callable(fh.Model.evaluate_fold_in)
    assert fh.EVAL_K_LIST == (5, 10, 20, 50, 100)
    assert np.allclose(fh.EVAL_ALPHA_LIST, MR.DEFAULT_ALPHAS)
