"""Model.evaluate / Model.evaluate_fold_in (include/frecsys_model.h): the
device evaluation behind the model classes.

test_model_equals_parts   iALS and SAFER2 on the quirk data: the per-user
                          arrays are bitwise list_metrics of the model's own
                          recommend lists; the summary means are the double
                          sums in row order; the summary CVaRs are bitwise
                          metric_cvar of the columns (EvaluationResult::cvar
                          and its C restatement pinned to each other); the
                          EVAL side holds the projected rows afterwards.
test_gate_ials_evaluate   the reference's quality gate (ials_test.cc:17-45,
                          Mean NDCG@20 >= 0.2 on the ML-1M validation fold)
                          through the new API.
test_weighted_models      ERM-MF and CVaR-MF construct and evaluate.
"""
import numpy as np
import pytest

import metrics_ref as MR
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

K_LIST = fh.EVAL_K_LIST
ALPHAS = fh.EVAL_ALPHA_LIST


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _quirk_model(name, epochs, **flags):
    nu, ni, up, uc, _, _ = make_quirk_data()
    users = np.repeat(np.arange(nu), np.diff(up)).astype(np.int32)
    m = fh.Model(name, users, uc, dim=16, stdev=0.1, seed=1, l2_reg=0.003, uobs_weight=0.1,
                 print_train_stats=False, use_snr=False, **flags)
    assert (m.n_users, m.n_items) == (nu, ni)
    m.initialize()
    m.train(epochs)
    return m, up, uc


def _fold_in_rows(up, uc, users):
    """The histories of `users` as a fold-in CSR."""
    hp = np.concatenate([[0], np.cumsum([up[u + 1] - up[u] for u in users])]).astype(np.int64)
    hc = np.concatenate([uc[up[u]:up[u + 1]] for u in users]).astype(np.int32)
    return hp, hc


def _check_summary(ev, n):
    rec, ndcg = ev["recall"], ev["ndcg"]
    assert rec.shape == ndcg.shape == (n, len(K_LIST))
    assert ev["recall_cvar"].shape == ev["ndcg_cvar"].shape == (len(ALPHAS), len(K_LIST))
    for name, a in (("recall", rec), ("ndcg", ndcg)):
        for q in range(len(K_LIST)):
            s = 0.0
            for x in a[:, q]:   # row order, in double (types.h colwise().mean())
                s += float(x)
            assert _bits(ev["mean_" + name][q]) == _bits(np.float32(s / n)), (name, q)
            np.testing.assert_array_equal(_bits(ev[name + "_cvar"][:, q]),
                                          _bits(fh.metric_cvar(a[:, q], ALPHAS)))
            np.testing.assert_array_equal(_bits(ev[name + "_cvar"][:, q]),
                                          _bits(MR.cvar_ref(a[:, q], ALPHAS)))


@pytest.mark.parametrize("name", ["ials", "safer2"])
def test_model_equals_parts(name):
    m, up, uc = _quirk_model(name, 2)
    ni = m.n_items
    ctx = m.context()
    # fold-in: 120 users with a history, as unseen users
    users = [u for u in range(130) if up[u + 1] > up[u]][:120]
    hp, hc = _fold_in_rows(up, uc, users)
    n = len(users)
    gp, gi = MR.ground_truth(n, ni, hp, hc, 21)
    ev = m.evaluate_fold_in(hp, hc, gp, gi)
    ctx.n[fh.SIDE_EVAL] = n
    E1 = ctx.get_embeddings(fh.SIDE_EVAL)
    assert np.abs(E1).max() > 0
    items, _ = m.recommend_fold_in(hp, hc, max(K_LIST))
    E2 = ctx.get_embeddings(fh.SIDE_EVAL)
    np.testing.assert_array_equal(E1.view(np.uint32), E2.view(np.uint32))
    hrec, hndcg = fh.list_metrics(items, gp, gi, K_LIST)
    np.testing.assert_array_equal(_bits(ev["recall"]), _bits(hrec))
    np.testing.assert_array_equal(_bits(ev["ndcg"]), _bits(hndcg))
    _check_summary(ev, n)
    # trained users: shuffled, repeated
    rng = np.random.default_rng(22)
    tu = rng.permutation(m.n_users)[:150]
    tu = np.concatenate([tu, tu[:9]])
    gp, gi = MR.ground_truth(tu, ni, up, uc, 23)
    for seen in (True, False):
        ev = m.evaluate(tu, gp, gi, exclude_seen=seen)
        items, _ = m.recommend(tu, max(K_LIST), exclude_seen=seen)
        hrec, hndcg = fh.list_metrics(items, gp, gi, K_LIST)
        np.testing.assert_array_equal(_bits(ev["recall"]), _bits(hrec))
        np.testing.assert_array_equal(_bits(ev["ndcg"]), _bits(hndcg))
        _check_summary(ev, len(tu))
    with pytest.raises(fh.FrecsysError) as ei:
        m.evaluate([0], [0, 1], [ni])
    assert ei.value.code == fh.ERR_INVALID
    with pytest.raises(fh.FrecsysError) as ei:
        m.evaluate_fold_in([0, 1], [3], [0, 0], np.zeros(0, np.int32))
    assert ei.value.code == fh.ERR_INVALID
    m.close()


def test_gate_ials_evaluate(ml1m):  # ials_test.cc:17-45
    tr, vt, ve = ml1m
    m = fh.Model("ials", tr.users, tr.items, dim=8, uobs_weight=0.1, l2_reg=0.003, seed=1,
                 print_train_stats=False)
    m.initialize()
    m.train(10)
    ids, ep, ec = vt.compact_users()
    te_ids, tp, tc = ve.compact_users()
    row_of = {int(u): r for r, u in enumerate(ids)}
    assert all(int(u) in row_of for u in te_ids)
    rows = [row_of[int(u)] for u in te_ids]
    hp = np.concatenate([[0], np.cumsum([ep[r + 1] - ep[r] for r in rows])]).astype(np.int64)
    hc = np.concatenate([ec[ep[r]:ep[r + 1]] for r in rows]).astype(np.int32)
    assert tc.max() < m.n_items and np.all(np.diff(tp) > 0)
    ev = m.evaluate_fold_in(hp, hc, tp, tc)
    q = list(K_LIST).index(20)
    print(f"iALS ML-1M fold-in evaluation, {len(te_ids)} users: mean NDCG@20 "
          f"{ev['mean_ndcg'][q]:.4f}, mean Recall@20 {ev['mean_recall'][q]:.4f}, "
          f"NDCG CVaR(0.3)@20 {ev['ndcg_cvar'][2, q]:.4f}")
    assert ev["mean_ndcg"][q] >= 0.2
    m.close()


@pytest.mark.parametrize("name", ["erm_mf", "cvar_mf"])
def test_weighted_models(name):
    m, up, uc = _quirk_model(name, 1, stepsize=0.4)
    users = [u for u in range(70) if up[u + 1] > up[u]][:60]
    hp, hc = _fold_in_rows(up, uc, users)
    gp, gi = MR.ground_truth(len(users), m.n_items, hp, hc, 31)
    ev = m.evaluate_fold_in(hp, hc, gp, gi)
    items, _ = m.recommend_fold_in(hp, hc, max(K_LIST))
    hrec, hndcg = fh.list_metrics(items, gp, gi, K_LIST)
    np.testing.assert_array_equal(_bits(ev["recall"]), _bits(hrec))
    np.testing.assert_array_equal(_bits(ev["ndcg"]), _bits(hndcg))
    assert np.isfinite(ev["ndcg"]).all() and np.isfinite(ev["mean_ndcg"]).all()
    ev = m.evaluate(np.arange(40), *MR.ground_truth(40, m.n_items, up, uc, 32))
    assert ev["recall"].shape == (40, len(K_LIST)) and np.isfinite(ev["recall"]).all()
    m.close()
