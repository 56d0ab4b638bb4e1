"""Model.recommend_diverse / recommend_diverse_fold_in / diversify
(include/frecsys_model.h) on the ML-1M golden files: iALS at dim 64 after three
epochs.

lam = 1 returns Model.recommend's lists; lam = 0.5 returns fh.mmr_select of
the pool Model.recommend(users, pool) returns against the model's item table,
byte for byte -- for trained users, for fold-in users, and from a loaded
checkpoint.  Sanity, no tolerance: the lam = 0.5 lists are less alike among
themselves (mean pairwise cosine, float64) than the lam = 1 lists.
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
    m.train(3)
    yield m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    assert len(got) == len(want)
    np.testing.assert_array_equal(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(_bits(g), _bits(w))


def _mean_pairwise_cosine(V, lists):
    V64 = V.astype(np.float64)
    V64 = V64 / np.maximum(np.linalg.norm(V64, axis=1, keepdims=True), 1e-300)
    out = []
    for row in lists:
        R = V64[row[row >= 0]]
        C = R @ R.T
        n = len(R)
        out.append((C.sum() - np.trace(C)) / (n * (n - 1)))
    return float(np.mean(out))


def test_trained_users(model):
    m = model
    V = m.context().get_embeddings(fh.SIDE_ITEM)
    rng = np.random.default_rng(21)
    users = np.concatenate([[0, m.n_users - 1], rng.permutation(m.n_users)[:300]])
    assert fh.default_pool(K) == POOL
    _same(m.recommend_diverse(users, K, lam=1.0), m.recommend(users, K))
    pool_i, pool_s = m.recommend(users, POOL)
    for raw in (False, True):
        got = m.recommend_diverse(users, K, lam=0.5, raw_scores=raw, return_mmr=True)
        want = fh.mmr_select(V, pool_i, pool_s, K, 0.5, raw_scores=raw, return_mmr=True)
        _same(got, want)
        _same(m.diversify(pool_i, pool_s, K, 0.5, raw_scores=raw, return_mmr=True), want)
    # a pool of another size, the history kept, a mask
    mask = (rng.random(m.n_items) < 0.5).astype(np.uint8)
    got = m.recommend_diverse(users, 10, pool=33, lam=0.3, exclude_history=False, item_mask=mask)
    pi, ps = m.recommend(users, 33, exclude_seen=False, item_mask=mask)
    _same(got, fh.mmr_select(V, pi, ps, 10, 0.3))
    top = m.recommend(users, K)[0]
    div = m.recommend_diverse(users, K, lam=0.5)[0]
    c_top, c_div = _mean_pairwise_cosine(V, top), _mean_pairwise_cosine(V, div)
    print(f"mean pairwise cosine: top-{K} {c_top:.4f}, lam=0.5 {c_div:.4f}")
    assert c_div < c_top


def test_fold_in_users(model, ml1m):
    m = model
    _, vt, _ = ml1m
    _, ep, ec = vt.compact_users()
    n = 200
    ep, ec = ep[:n + 1], ec[:ep[n]]
    V = m.context().get_embeddings(fh.SIDE_ITEM)
    _same(m.recommend_diverse_fold_in(ep, ec, K, lam=1.0), m.recommend_fold_in(ep, ec, K))
    pool_i, pool_s = m.recommend_fold_in(ep, ec, POOL)
    got = m.recommend_diverse_fold_in(ep, ec, K, lam=0.5, return_mmr=True)
    _same(got, fh.mmr_select(V, pool_i, pool_s, K, 0.5, return_mmr=True))
    with pytest.raises(fh.FrecsysError) as ei:
        m.recommend_diverse_fold_in(ep, ec, K, pool=K - 1)
    assert ei.value.code == fh.ERR_INVALID


def test_saved_and_loaded(model, tmp_path):
    m = model
    users = np.arange(0, m.n_users, 37)
    want = m.recommend_diverse(users, K, lam=0.5, return_mmr=True)
    path = str(tmp_path / "model.frm")
    m.save(path)
    b = fh.Model.load(path)
    try:
        _same(b.recommend_diverse(users, K, lam=0.5, return_mmr=True), want)
    finally:
        b.close()


def test_bad_arguments_raise(model):
    m = model
    for kw in (dict(k=0), dict(k=K, pool=K - 1), dict(k=K, pool=1025), dict(k=K, lam=1.5),
               dict(k=K, lam=float("nan"))):
        with pytest.raises(fh.FrecsysError) as ei:
            m.recommend_diverse([0, 1], **kw)
        assert ei.value.code == fh.ERR_INVALID, kw
    with pytest.raises(fh.FrecsysError) as ei:
        m.diversify(np.full((1, 4), m.n_items, np.int32), np.zeros((1, 4), np.float32), 2)
    assert ei.value.code == fh.ERR_INVALID
    items, scores = m.recommend_diverse([], K)
    assert items.shape == scores.shape == (0, K)
