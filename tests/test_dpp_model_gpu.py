"""Model.recommend_dpp / recommend_dpp_fold_in / diversify_dpp
(include/frecsys_model.h) on the ML-1M golden files: iALS at dim 64 after one
epoch.

Each returns fh.dpp_select of the pool Model.recommend(users, pool) returns
against the model's item table, and the context path's result, byte for byte --
for trained users, for fold-in users, from a loaded checkpoint and from a
serve-only one.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

DIM, K, POOL = 64, 20, 80


@pytest.fixture(scope="module")
def model(ml1m):
    tr, _, _ = ml1m
    m = fh.Model("ials", tr.users, tr.items, dim=DIM, stdev=0.1, seed=1, l2_reg=0.003,
                 l2_reg_exp=1.0, uobs_weight=0.1, print_train_stats=False)
    m.initialize()
    m.train(1)
    yield m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    assert len(got) == len(want)
    np.testing.assert_array_equal(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(_bits(g), _bits(w))


def test_trained_users(model):
    m = model
    ctx = m.context()
    V = ctx.get_embeddings(fh.SIDE_ITEM)
    rng = np.random.default_rng(31)
    users = np.concatenate([[0, m.n_users - 1], rng.permutation(m.n_users)[:200]])
    assert fh.default_pool(K) == POOL
    pool_i, pool_s = m.recommend(users, POOL)
    for raw, theta in ((False, 4.0), (True, 1.0), (False, 0.0)):
        got = m.recommend_dpp(users, K, theta=theta, raw_scores=raw, return_gain=True)
        want = fh.dpp_select(V, pool_i, pool_s, K, theta, 1e-3, raw_scores=raw, return_gain=True)
        _same(got, want)
        _same(m.diversify_dpp(pool_i, pool_s, K, theta, raw_scores=raw, return_gain=True), want)
        _same(ctx.recommend_dpp(fh.SIDE_USER, K, POOL, theta, rows=users, raw_scores=raw,
                                return_gain=True), want)
        _same(ctx.diversify_dpp(pool_i, pool_s, K, theta, raw_scores=raw, return_gain=True), want)
    # a pool of another size, the history kept, a mask, another eps
    mask = (rng.random(m.n_items) < 0.5).astype(np.uint8)
    got = m.recommend_dpp(users, 10, pool=33, theta=2.0, eps=0.05, exclude_seen=False,
                          item_mask=mask)
    pi, ps = m.recommend(users, 33, exclude_seen=False, item_mask=mask)
    _same(got, fh.dpp_select(V, pi, ps, 10, 2.0, 0.05))


def test_fold_in_users(model, ml1m):
    m = model
    _, vt, _ = ml1m
    _, ep, ec = vt.compact_users()
    n = 200
    ep, ec = ep[:n + 1], ec[:ep[n]]
    V = m.context().get_embeddings(fh.SIDE_ITEM)
    pool_i, pool_s = m.recommend_fold_in(ep, ec, POOL)
    got = m.recommend_dpp_fold_in(ep, ec, K, return_gain=True)
    _same(got, fh.dpp_select(V, pool_i, pool_s, K, return_gain=True))
    # the projected rows stay in the EVAL side: the context path on them
    _same(m.context().recommend_dpp(fh.SIDE_EVAL, K, POOL, rows=np.arange(n), return_gain=True),
          got)
    with pytest.raises(fh.FrecsysError) as ei:
        m.recommend_dpp_fold_in(ep, ec, K, pool=K - 1)
    assert ei.value.code == fh.ERR_INVALID


def test_saved_loaded_and_serve_only(model, ml1m, tmp_path):
    m = model
    _, vt, _ = ml1m
    _, ep, ec = vt.compact_users()
    ep, ec = ep[:51], ec[:ep[50]]
    users = np.arange(0, m.n_users, 37)
    want = m.recommend_dpp(users, K, return_gain=True)
    kept = m.recommend_dpp(users, K, exclude_seen=False, return_gain=True)
    fold = m.recommend_dpp_fold_in(ep, ec, K, return_gain=True)
    full, serve = str(tmp_path / "model.frm"), str(tmp_path / "serve.frm")
    m.save(full)
    m.save(serve, include_data=False)
    b = fh.Model.load(full)
    try:
        _same(b.recommend_dpp(users, K, return_gain=True), want)
        _same(b.recommend_dpp_fold_in(ep, ec, K, return_gain=True), fold)
    finally:
        b.close()
    s = fh.Model.load(serve)
    try:
        with pytest.raises(fh.FrecsysError) as ei:
            s.recommend_dpp(users, K)  # exclude_seen needs the training tuples
        assert ei.value.code == fh.ERR_INVALID and "serve-only" in str(ei.value)
        _same(s.recommend_dpp(users, K, exclude_seen=False, return_gain=True), kept)
        _same(s.recommend_dpp_fold_in(ep, ec, K, return_gain=True), fold)
        pi, ps = s.recommend(users, POOL, exclude_seen=False)
        _same(s.diversify_dpp(pi, ps, K, return_gain=True), kept)
    finally:
        s.close()


def test_bad_arguments_raise(model):
    m = model
    for kw in (dict(k=0), dict(k=K, pool=K - 1), dict(k=K, pool=1025), dict(k=K, theta=-1.0),
               dict(k=K, theta=float("nan")), dict(k=K, eps=0.0), dict(k=K, eps=2.0)):
        with pytest.raises(fh.FrecsysError) as ei:
            m.recommend_dpp([0, 1], **kw)
        assert ei.value.code == fh.ERR_INVALID, kw
    with pytest.raises(fh.FrecsysError) as ei:
        m.diversify_dpp(np.full((1, 4), m.n_items, np.int32), np.zeros((1, 4), np.float32), 2)
    assert ei.value.code == fh.ERR_INVALID
    items, scores = m.recommend_dpp([], K)
    assert items.shape == scores.shape == (0, K)
