"""Model.score / Model.rank_candidates / Model.rank_candidates_fold_in
(include/frecsys_model.h) on the ML-1M golden files at dim 32 after 2 epochs,
for iALS and SAFER2.

Trained users: Model.rank_candidates is bitwise Context.rank_candidates on the
model's own context, and Model.score returns the bits Model.recommend lists.
Fold-in users (validation_tr): rank_candidates_fold_in is bitwise the ranking
of the same projection made by hand on the same context.  exclude_seen drops
the training history of trained users and the given history of fold-in users.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

DIM, EPOCHS, K = 32, 2, 20
REG, W = 0.003, 0.1
MODELS = ("ials", "safer2")
LIST = 200

_models = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _model(name, tr):
    if name not in _models:
        m = fh.Model(name, tr.users, tr.items, dim=DIM, stdev=0.1, seed=1, l2_reg=REG,
                     l2_reg_exp=1.0, uobs_weight=W, print_train_stats=False, use_snr=False)
        m.initialize()
        m.train(EPOCHS)
        _models[name] = m
    return _models[name]


def _lists(rng, ptr, col, rows, n_items):
    """Per row LIST candidate ids, up to half of them from the row's own history."""
    out = []
    for r in rows:
        h = col[ptr[r]:ptr[r + 1]]
        own = rng.choice(h, min(len(h), LIST // 2), replace=False) if len(h) else h[:0]
        out.append(np.concatenate([own, rng.integers(0, n_items, LIST - len(own))]).astype(np.int32))
    return (LIST * np.arange(len(out) + 1)).astype(np.int64), np.concatenate(out)


@pytest.mark.parametrize("name", MODELS)
def test_trained_users(ml1m, name):
    tr, _, _ = ml1m
    m = _model(name, tr)
    ctx = m.context()
    up, uc = tr.by_user()
    rng = np.random.default_rng(23)
    users = rng.permutation(m.n_users)[:300]
    users = np.concatenate([users, users[:7]])
    cp, ci = _lists(rng, up, uc, users, m.n_items)
    mask = (rng.random(m.n_items) < 0.5).astype(np.uint8)
    for exclude, mk in ((True, None), (False, None), (True, mask)):
        it, sc = m.rank_candidates(users, cp, ci, K, exclude_seen=exclude, item_mask=mk)
        ci_, cs_ = ctx.rank_candidates(fh.SIDE_USER, K, cp, ci, rows=users,
                                       exclude_history=exclude, item_mask=mk)
        assert it.shape == sc.shape == (len(users), K)
        np.testing.assert_array_equal(it, ci_)
        np.testing.assert_array_equal(_bits(sc), _bits(cs_))
        seen = [bool(set(it[i].tolist()) & set(uc[up[u]:up[u + 1]].tolist()))
                for i, u in enumerate(users)]
        assert not any(seen) if exclude else any(seen)
        if mk is not None:
            assert mask[it[it >= 0]].all()
    # the scores recommend lists, pair by pair
    ri, rs = m.recommend(users, K)
    p = rng.permutation(ri.size)
    got = m.score(np.repeat(users, K)[p], ri.reshape(-1)[p])
    np.testing.assert_array_equal(_bits(got), _bits(rs.reshape(-1)[p]))
    with pytest.raises(fh.FrecsysError) as ei:
        m.score([m.n_users], [0])
    assert ei.value.code == fh.ERR_INVALID
    with pytest.raises(fh.FrecsysError) as ei:
        m.rank_candidates([0], [0, 1], [m.n_items], K)
    assert ei.value.code == fh.ERR_INVALID


def _fold_in_by_hand(name, ctx, ep, ec):
    ctx.load_csr(fh.SIDE_EVAL, ep, ec)
    if name == "ials":
        ctx.gramian(fh.SIDE_ITEM, fetch=False)
        ctx.solve_side(fh.SIDE_EVAL, fh.KIND_IALS, REG, W, reg_exp=1.0)
    else:  # StepU with omega = 1 and the item Gramian Train() left
        ctx.solve_side(fh.SIDE_EVAL, fh.KIND_WEIGHTED_U, REG, W)


@pytest.mark.parametrize("name", MODELS)
def test_fold_in_users(ml1m, name):
    tr, vt, _ = ml1m
    m = _model(name, tr)
    ids, ep, ec = vt.compact_users()
    n = len(ids)
    rng = np.random.default_rng(29)
    cp, ci = _lists(rng, ep, ec, np.arange(n), m.n_items)
    it, sc = m.rank_candidates_fold_in(ep, ec, cp, ci, K)
    assert it.shape == sc.shape == (n, K) and (it >= 0).any()
    for r in range(n):   # the given history is dropped
        assert not set(it[r].tolist()) & set(ec[ep[r]:ep[r + 1]].tolist())
    it2, _ = m.rank_candidates_fold_in(ep, ec, cp, ci, K, exclude_seen=False)
    assert any(set(it2[r].tolist()) & set(ec[ep[r]:ep[r + 1]].tolist()) for r in range(n))
    ctx = m.context()
    ctx.n[fh.SIDE_EVAL] = n
    _fold_in_by_hand(name, ctx, ep, ec)
    hi, hs = ctx.rank_candidates(fh.SIDE_EVAL, K, cp, ci)
    np.testing.assert_array_equal(it, hi)
    np.testing.assert_array_equal(_bits(sc), _bits(hs))
    with pytest.raises(fh.FrecsysError) as ei:
        m.rank_candidates_fold_in(ep, ec, cp, np.where(ci == ci[0], m.n_items, ci), K)
    assert ei.value.code == fh.ERR_INVALID
