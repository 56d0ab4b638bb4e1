"""Model.recommend / Model.recommend_fold_in (include/frecsys_model.h) on the
ML-1M golden files at dim 32 after 2 epochs, for iALS, SAFER2 and iALS++.

Trained users: the lists against float64 scores of the model's own tables by
the tolerant rule of test_topk_gpu._check (no exactness claim on real data:
no history item listed, scores non-increasing within 2e-6 max|S|, every item
better than the k-th by more than that present).

Fold-in users (validation_tr): the EVAL embeddings recommend_fold_in leaves
are bitwise those of the same projection made by hand on the same context --
solve_side(SIDE_EVAL) with the model's parameters, or iALS++'s 8 epochs of
block steps -- and the lists pass the tolerant rule.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

DIM, EPOCHS, K = 32, 2, 20
REG, W, BLOCK = 0.003, 0.1, 16
MODELS = ("ials", "safer2", "ialspp")

_models = {}


def _model(name, tr):
    if name not in _models:
        m = fh.Model(name, tr.users, tr.items, dim=DIM, stdev=0.1, seed=1, l2_reg=REG,
                     l2_reg_exp=1.0, uobs_weight=W, block_size=BLOCK, print_train_stats=False,
                     use_snr=False)
        m.initialize()
        m.train(EPOCHS)
        _models[name] = m
    return _models[name]


def _check_lists(items, scores, S, ptr, col, rows, k):
    """items / scores [n, k] for the CSR rows `rows` against float64 S [n, m]."""
    tol = 2e-6 * np.abs(S).max()
    for i, r in enumerate(rows):
        t = items[i]
        hist = col[ptr[r]:ptr[r + 1]]
        assert (t >= 0).all() and len(set(t.tolist())) == k, i
        assert not set(t.tolist()) & set(hist.tolist()), i
        st = S[i, t]
        assert np.all(np.diff(st) <= tol), i
        assert np.all(np.abs(scores[i] - st) <= tol), i
        free = S[i].copy()
        free[hist] = -np.inf
        kth = -np.partition(-free, k - 1)[k - 1]
        must = set(np.nonzero(free > kth + tol)[0].tolist())
        assert must <= set(t.tolist()), i
        assert np.all(st >= kth - tol), i


@pytest.mark.parametrize("name", MODELS)
def test_recommend_trained_users(ml1m, name):
    tr, _, _ = ml1m
    m = _model(name, tr)
    ctx = m.context()
    U = ctx.get_embeddings(fh.SIDE_USER).astype(np.float64)
    V = ctx.get_embeddings(fh.SIDE_ITEM).astype(np.float64)
    up, uc = tr.by_user()
    rng = np.random.default_rng(3)
    users = rng.permutation(m.n_users)[:400]
    users = np.concatenate([users, users[:7]])
    items, scores = m.recommend(users, K)
    assert items.shape == scores.shape == (len(users), K)
    _check_lists(items, scores, U[users] @ V.T, up, uc, users, K)
    # seen items come back once the exclusion is off, for some user
    it2, _ = m.recommend(users[:50], K, exclude_seen=False)
    assert any(set(it2[i].tolist()) & set(uc[up[u]:up[u + 1]].tolist())
               for i, u in enumerate(users[:50]))
    # a mask keeps the lists inside it
    mask = (rng.random(m.n_items) < 0.5).astype(np.uint8)
    it3, _ = m.recommend(users[:50], K, item_mask=mask)
    assert mask[it3].all()
    with pytest.raises(fh.FrecsysError) as ei:
        m.recommend([m.n_users], K)
    assert ei.value.code == fh.ERR_INVALID


def _fold_in_by_hand(name, ctx, ep, ec):
    ctx.load_csr(fh.SIDE_EVAL, ep, ec)
    if name == "ials":
        ctx.gramian(fh.SIDE_ITEM, fetch=False)
        ctx.solve_side(fh.SIDE_EVAL, fh.KIND_IALS, REG, W, reg_exp=1.0)
    elif name == "safer2":  # StepU with omega = 1 and the item Gramian Train() left
        ctx.solve_side(fh.SIDE_EVAL, fh.KIND_WEIGHTED_U, REG, W)
    else:  # ialspp.h:148-206
        ctx.set_embeddings(fh.SIDE_EVAL, np.zeros((len(ep) - 1, DIM), np.float32))
        for _ in range(8):
            ctx.pp_predict(fh.SIDE_EVAL)
            for start in range(0, DIM, BLOCK):
                ctx.gramian(fh.SIDE_ITEM, fetch=False)
                ctx.pp_step(fh.SIDE_EVAL, start, min(start + BLOCK, DIM), REG, W, reg_exp=1.0)
    return ctx.get_embeddings(fh.SIDE_EVAL)


@pytest.mark.parametrize("name", MODELS)
def test_recommend_fold_in_users(ml1m, name):
    tr, vt, _ = ml1m
    m = _model(name, tr)
    ids, ep, ec = vt.compact_users()
    n = len(ids)
    items, scores = m.recommend_fold_in(ep, ec, K)
    assert items.shape == scores.shape == (n, K)
    ctx = m.context()
    ctx.n[fh.SIDE_EVAL] = n
    E = ctx.get_embeddings(fh.SIDE_EVAL)
    assert np.abs(E).max() > 0
    V = ctx.get_embeddings(fh.SIDE_ITEM).astype(np.float64)
    _check_lists(items, scores, E.astype(np.float64) @ V.T, ep, ec, np.arange(n), K)
    Eh = _fold_in_by_hand(name, ctx, ep, ec)
    np.testing.assert_array_equal(E.view(np.uint32), Eh.view(np.uint32))
