"""Model.evaluate_ranks / Model.evaluate_ranks_fold_in
(include/frecsys_model.h) on the ML-1M fold of tests/golden: iALS, dim 16, one
epoch.

test_ranks_equal_recommend_positions  every rank below 1024 is the place of
                          that item in Model.recommend(k = 1024)'s list, and
                          every listed ground-truth item has that rank.
test_recall_rebuilt_from_ranks        Recall@K rebuilt from the ranks equals
                          Model.evaluate's, bitwise, at every default cut-off.
test_fold_in_equals_context           the fold-in form equals
                          Context.rank_positions on the EVAL rows it leaves.
test_summary                          the means are float64 row-order means,
                          the CVaRs fh.metric_cvar of the per-user arrays.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

K_LIST = fh.EVAL_K_LIST
ALPHAS = fh.EVAL_ALPHA_LIST
_state = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _setup(ml1m):
    """The model, and the held-out users as fold-in histories with their
    ground truth; shared by the tests and left unchanged."""
    if not _state:
        tr, vt, ve = ml1m
        m = fh.Model("ials", tr.users, tr.items, dim=16, uobs_weight=0.1, l2_reg=0.003, seed=1,
                     print_train_stats=False)
        m.initialize()
        m.train(1)
        ids, ep, ec = vt.compact_users()
        te_ids, tp, tc = ve.compact_users()
        row_of = {int(u): r for r, u in enumerate(ids)}
        rows = [row_of[int(u)] for u in te_ids]
        hp = np.concatenate([[0], np.cumsum([ep[r + 1] - ep[r] for r in rows])]).astype(np.int64)
        hc = np.concatenate([ec[ep[r]:ep[r + 1]] for r in rows]).astype(np.int32)
        assert tc.max() < m.n_items and np.all(np.diff(tp) > 0)
        # trained users: a shuffled subset with repeats; their ground truth is
        # the held-out users' (any ids do: the ranking is what is compared)
        rng = np.random.default_rng(3)
        n = min(300, len(te_ids))
        users = rng.permutation(m.n_users)[:n]
        users[-3:] = users[:3]
        _state.update(m=m, hp=hp, hc=hc, tp=tp.astype(np.int64), tc=tc.astype(np.int32),
                      users=users.astype(np.int64), up=tp[:n + 1].astype(np.int64),
                      uc=tc[:tp[n]].astype(np.int32))
    return _state


@pytest.mark.parametrize("seen", [True, False])
def test_ranks_equal_recommend_positions(ml1m, seen):
    s = _setup(ml1m)
    m, users, gp, gi = s["m"], s["users"], s["up"], s["uc"]
    ev = m.evaluate_ranks(users, gp, gi, exclude_seen=seen)
    items, _ = m.recommend(users, 1024, exclude_seen=seen)
    rank = ev["rank"]
    assert rank.shape == gi.shape and ev["eligible"].shape == (len(users),)
    for i in range(len(users)):
        pos = np.full(m.n_items, -2, np.int64)  # -2: eligible or not, not in the first 1024
        pos[items[i][items[i] >= 0]] = np.arange((items[i] >= 0).sum())
        r = rank[gp[i]:gp[i + 1]]
        g = gi[gp[i]:gp[i + 1]]
        below = (r >= 0) & (r < 1024)
        np.testing.assert_array_equal(r[below], pos[g[below]])
        np.testing.assert_array_equal(pos[g] >= 0, below)
    assert (rank >= 1024).any(), "the fold must reach past the lists, or the test shows nothing"
    assert (ev["eligible"] <= m.n_items).all() and (rank < ev["eligible"].max()).all()
    if not seen:
        assert (ev["eligible"] == m.n_items).all() and (rank >= 0).all()


def test_recall_rebuilt_from_ranks(ml1m):
    s = _setup(ml1m)
    m, users, gp, gi = s["m"], s["users"], s["up"], s["uc"]
    ev = m.evaluate(users, gp, gi)
    rk = m.evaluate_ranks(users, gp, gi)["rank"]
    rebuilt = np.zeros_like(ev["recall"])
    for i in range(len(users)):
        r = rk[gp[i]:gp[i + 1]]
        g = len(set(gi[gp[i]:gp[i + 1]].tolist()))
        distinct = np.unique(r[r >= 0])
        for q, k in enumerate(K_LIST):
            hits = int((distinct < k).sum())
            rebuilt[i, q] = np.float32(np.float64(hits) / np.float64(np.float32(min(k, g))))
    np.testing.assert_array_equal(_bits(rebuilt), _bits(ev["recall"]))
    assert rebuilt.any()


def test_fold_in_equals_context(ml1m):
    s = _setup(ml1m)
    m, hp, hc, tp, tc = s["m"], s["hp"], s["hc"], s["tp"], s["tc"]
    n = len(hp) - 1
    mask = (np.random.default_rng(4).random(m.n_items) < 0.8).astype(np.uint8)
    for seen, mk in ((True, None), (False, mask)):
        ev = m.evaluate_ranks_fold_in(hp, hc, tp, tc, exclude_seen=seen, item_mask=mk)
        ctx = m.context()
        ctx.n[fh.SIDE_EVAL] = n
        rank, elig, mrr, auc = ctx.rank_positions(fh.SIDE_EVAL, tp, tc, exclude_history=seen,
                                                  item_mask=mk)
        np.testing.assert_array_equal(ev["rank"], rank)
        np.testing.assert_array_equal(ev["eligible"], elig)
        np.testing.assert_array_equal(_bits(ev["mrr"]), _bits(mrr))
        np.testing.assert_array_equal(_bits(ev["auc"]), _bits(auc))
        hm, ha = fh.position_metrics(rank, tp, elig)
        np.testing.assert_array_equal(_bits(mrr), _bits(hm))
        np.testing.assert_array_equal(_bits(auc), _bits(ha))
    print(f"iALS ML-1M d=16, 1 epoch, {n} fold-in users: mean MRR {ev['mean_mrr']:.4f}, "
          f"mean AUC {ev['mean_auc']:.4f}, deepest rank {int(ev['rank'].max())}")


def test_summary(ml1m):
    s = _setup(ml1m)
    m, hp, hc, tp, tc = s["m"], s["hp"], s["hc"], s["tp"], s["tc"]
    ev = m.evaluate_ranks_fold_in(hp, hc, tp, tc)
    n = len(hp) - 1
    assert ev["mrr_cvar"].shape == ev["auc_cvar"].shape == (len(ALPHAS),)
    for name in ("mrr", "auc"):
        tot = 0.0
        for x in ev[name]:  # row order, in double
            tot += float(x)
        assert _bits(np.float32(ev["mean_" + name])) == _bits(np.float32(tot / n)), name
        np.testing.assert_array_equal(_bits(ev[name + "_cvar"]),
                                      _bits(fh.metric_cvar(ev[name], ALPHAS)))
    assert 0.5 < ev["mean_auc"] <= 1.0 and 0.0 < ev["mean_mrr"] <= 1.0
    assert ev["auc_cvar"][0] < ev["mean_auc"]  # the tail is worse than the mean
    with pytest.raises(fh.FrecsysError) as ei:
        m.evaluate_ranks([0], [0, 1], [m.n_items])
    assert ei.value.code == fh.ERR_INVALID
    with pytest.raises(fh.FrecsysError) as ei:
        m.evaluate_ranks_fold_in([0, 1], [3], [0, 0], np.zeros(0, np.int32))
    assert ei.value.code == fh.ERR_INVALID
