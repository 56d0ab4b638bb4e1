"""Model.evaluate_sampled / Model.evaluate_candidates and their fold-in forms
(include/frecsys_model.h): bitwise the context calls they stand on, with
evaluate's summary arithmetic.

test_model_equals_context  iALS on the quirk data: trained users (shuffled,
                           repeated) and fold-in rows; the per-user arrays
                           equal Context.sampled_metrics /
                           Context.rank_candidates_metrics, the summary is
                           evaluate's (double means in row order, metric_cvar
                           of the columns).
test_model_bad_arguments   FRECSYS_ERR_INVALID before the fold-in projection.
"""
import numpy as np
import pytest

import metrics_ref as MR
import sampled_ref as SR
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

K_LIST = fh.EVAL_K_LIST
ALPHAS = fh.EVAL_ALPHA_LIST


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def model():
    nu, ni, up, uc, _, _ = make_quirk_data()
    users = np.repeat(np.arange(nu), np.diff(up)).astype(np.int32)
    m = fh.Model("ials", users, uc, dim=16, stdev=0.1, seed=1, l2_reg=0.003, uobs_weight=0.1,
                 print_train_stats=False)
    m.initialize()
    m.train(2)
    yield m, up, uc
    m.close()


def _check(ev, rec, ndcg):
    n = rec.shape[0]
    np.testing.assert_array_equal(_bits(ev["recall"]), _bits(rec))
    np.testing.assert_array_equal(_bits(ev["ndcg"]), _bits(ndcg))
    assert ev["recall_cvar"].shape == ev["ndcg_cvar"].shape == (len(ALPHAS), len(K_LIST))
    for name, a in (("recall", rec), ("ndcg", ndcg)):
        for q in range(len(K_LIST)):
            s = 0.0
            for x in a[:, q]:   # row order, in double: evaluate's mean
                s += float(x)
            assert _bits(ev["mean_" + name][q]) == _bits(np.float32(s / n)), (name, q)
            np.testing.assert_array_equal(_bits(ev[name + "_cvar"][:, q]),
                                          _bits(fh.metric_cvar(a[:, q], ALPHAS)))


def _lists(n, ni, gp, gi, seed):
    """Candidate lists: part of the row's ground truth, then random ids."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        g = gi[gp[i]:gp[i + 1]]
        out.append(np.concatenate([g[:max(1, len(g) // 2)],
                                   rng.integers(0, ni, int(rng.integers(0, 300)))]))
    return SR.csr(out)


def test_model_equals_context(model):
    m, up, uc = model
    ni, ctx = m.n_items, m.context()
    rng = np.random.default_rng(31)
    mask = (rng.random(ni) < 0.7).astype(np.uint8)
    # trained users: shuffled, repeated
    tu = rng.permutation(m.n_users)[:150]
    tu = np.concatenate([tu, tu[:9]])
    gp, gi = MR.ground_truth(tu, ni, up, uc, 32)
    cp, ci = _lists(len(tu), ni, gp, gi, 33)
    for seen, mk in ((True, None), (False, mask)):
        ev = m.evaluate_sampled(tu, gp, gi, 100, seed=5, exclude_seen=seen, item_mask=mk)
        rec, ndcg, cnt, _ = ctx.sampled_metrics(fh.SIDE_USER, K_LIST, gp, gi, 100, 5, rows=tu,
                                                exclude_history=seen, item_mask=mk,
                                                return_negatives=True)
        assert (cnt == 100).any()
        _check(ev, rec, ndcg)
        ev = m.evaluate_candidates(tu, cp, ci, gp, gi, exclude_seen=seen, item_mask=mk)
        rec, ndcg = ctx.rank_candidates_metrics(fh.SIDE_USER, K_LIST, cp, ci, gp, gi, rows=tu,
                                                exclude_history=seen, item_mask=mk)
        _check(ev, rec, ndcg)
        assert rec.max() > 0
    # n_neg >= items: the full-catalogue evaluation
    ev = m.evaluate_sampled(tu, gp, gi, ni, seed=1)
    full = m.evaluate(tu, gp, gi)
    for key in ("recall", "ndcg", "mean_recall", "mean_ndcg", "recall_cvar", "ndcg_cvar"):
        np.testing.assert_array_equal(_bits(ev[key]), _bits(full[key]))
    # fold-in: 120 users with a history, as unseen users
    users = [u for u in range(130) if up[u + 1] > up[u]][:120]
    hp, hc = SR.csr([uc[up[u]:up[u + 1]] for u in users])
    n = len(users)
    gp, gi = MR.ground_truth(n, ni, hp, hc, 34)
    cp, ci = _lists(n, ni, gp, gi, 35)
    ev = m.evaluate_sampled_fold_in(hp, hc, gp, gi, 50, seed=6, item_mask=mask)
    ctx.n[fh.SIDE_EVAL] = n
    E1 = ctx.get_embeddings(fh.SIDE_EVAL)
    assert np.abs(E1).max() > 0
    rec, ndcg = ctx.sampled_metrics(fh.SIDE_EVAL, K_LIST, gp, gi, 50, 6, item_mask=mask)
    _check(ev, rec, ndcg)
    ev = m.evaluate_candidates_fold_in(hp, hc, cp, ci, gp, gi, exclude_seen=False)
    np.testing.assert_array_equal(E1.view(np.uint32),
                                  ctx.get_embeddings(fh.SIDE_EVAL).view(np.uint32))
    rec, ndcg = ctx.rank_candidates_metrics(fh.SIDE_EVAL, K_LIST, cp, ci, gp, gi,
                                            exclude_history=False)
    _check(ev, rec, ndcg)
    items, _ = m.rank_candidates_fold_in(hp, hc, cp, ci, max(K_LIST), exclude_seen=False)
    hrec, hndcg = fh.list_metrics(items, gp, gi, K_LIST)
    np.testing.assert_array_equal(_bits(rec), _bits(hrec))
    np.testing.assert_array_equal(_bits(ndcg), _bits(hndcg))


def test_model_bad_arguments(model):
    m, up, uc = model
    ni = m.n_items
    ctx = m.context()
    ctx.timing_reset()

    def invalid(fn, *a, **kw):
        with pytest.raises(fh.FrecsysError) as ei:
            fn(*a, **kw)
        assert ei.value.code == fh.ERR_INVALID, ei.value

    invalid(m.evaluate_sampled, [0], [0, 1], [ni], 5)
    invalid(m.evaluate_sampled, [0], [0, 1], [1], -1)
    invalid(m.evaluate_sampled, [m.n_users], [0, 1], [1], 5)
    invalid(m.evaluate_sampled, [0], [0, 0], [], 5)
    invalid(m.evaluate_sampled, [0], [0, 1], [1], 5, k_list=[0])
    invalid(m.evaluate_sampled_fold_in, [0, 1], [ni], [0, 1], [1], 5)
    invalid(m.evaluate_sampled_fold_in, [0, 1], [3], [0, 1], [1], -1)
    invalid(m.evaluate_sampled_fold_in, [0, 1], [3], [0, 0], np.zeros(0, np.int32), 5)
    invalid(m.evaluate_candidates, [0], [0, 1], [ni], [0, 1], [1])
    invalid(m.evaluate_candidates, [0], [1, 2], [1, 2], [0, 1], [1])
    invalid(m.evaluate_candidates, [0], [0, 1], [1], [0, 1], [-1])
    invalid(m.evaluate_candidates_fold_in, [0, 1], [3], [0, 1], [ni], [0, 1], [1])
    invalid(m.evaluate_candidates_fold_in, [0, 1], [3], [0, 1], [1], [0, 0], np.zeros(0, np.int32))
    invalid(m.evaluate_candidates_fold_in, [0, 2], [3, -1], [0, 1], [1], [0, 1], [1])
    for key in ("sample_negatives", "rank_candidates", "rank_metrics", "solve_eval"):
        assert ctx.timing(key)[1] == 0, key
    ev = m.evaluate_sampled([0, 1], [0, 1, 2], [1, 2], 5)
    assert ev["recall"].shape == (2, len(K_LIST))
