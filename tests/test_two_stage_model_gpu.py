"""Model.recommend_two_stage / recommend_two_stage_fold_in
(include/frecsys_model.h) on the ML-1M golden files: iALS at dim 64 after one
epoch (G9).  With the fallback on (the default) both return Model.recommend's /
recommend_fold_in's lists bit for bit, whatever share of the rows stage 2
certifies on a trained table; that share is printed.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import frecsys_hip as fh  # noqa: E402

DIM, K = 64, 20


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
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))


def test_trained_users(model):
    m = model
    rng = np.random.default_rng(41)
    users = np.concatenate([[0, m.n_users - 1], rng.permutation(m.n_users)[:300]])
    want = m.recommend(users, K)
    items, scores, cert = m.recommend_two_stage(users, K)
    _same((items, scores), want)
    assert set(np.unique(cert)) <= {1, 2}
    print(f"two-stage certified share, ML-1M iALS d={DIM}, k={K}, default pool: "
          f"{float((cert == 1).mean()):.3f}")
    # without the fallback: the certified rows are recommend's, the bytes agree
    i0, s0, c0 = m.recommend_two_stage(users, K, exact=False)
    np.testing.assert_array_equal(c0 == 1, cert == 1)
    c = c0 == 1
    _same((i0[c], s0[c]), (want[0][c], want[1][c]))
    # the context path, another pool, the history kept, a mask
    mask = (rng.random(m.n_items) < 0.5).astype(np.uint8)
    got = m.recommend_two_stage(users, 10, pool=200, exclude_seen=False, item_mask=mask)
    _same(got[:2], m.recommend(users, 10, exclude_seen=False, item_mask=mask))
    _same(m.context().recommend_two_stage(fh.SIDE_USER, 10, 200, rows=users,
                                          exclude_history=False, item_mask=mask)[:2], got[:2])


def test_fold_in_users(model, ml1m):
    m = model
    _, vt, _ = ml1m
    _, ep, ec = vt.compact_users()
    n = 200
    ep, ec = ep[:n + 1], ec[:ep[n]]
    want = m.recommend_fold_in(ep, ec, K)
    got = m.recommend_two_stage_fold_in(ep, ec, K)
    _same(got[:2], want)
    print(f"two-stage certified share, ML-1M fold-in: {float((got[2] == 1).mean()):.3f}")
    for kw in (dict(k=0), dict(k=K, pool=K - 1), dict(k=K, pool=1025)):
        with pytest.raises(fh.FrecsysError) as ei:
            m.recommend_two_stage_fold_in(ep, ec, **kw)
        assert ei.value.code == fh.ERR_INVALID, kw
        with pytest.raises(fh.FrecsysError) as ei:
            m.recommend_two_stage([0, 1], **kw)
        assert ei.value.code == fh.ERR_INVALID, kw
    items, scores, cert = m.recommend_two_stage([], K)
    assert items.shape == scores.shape == (0, K) and cert.shape == (0,)


def test_serve_only(model, tmp_path):
    m = model
    users = np.arange(0, m.n_users, 37)
    kept = m.recommend(users, K, exclude_seen=False)
    serve = str(tmp_path / "serve.frm")
    m.save(serve, include_data=False)
    s = fh.Model.load(serve)
    try:
        with pytest.raises(fh.FrecsysError) as ei:
            s.recommend_two_stage(users, K)  # exclude_seen needs the training tuples
        assert ei.value.code == fh.ERR_INVALID and "serve-only" in str(ei.value)
        _same(s.recommend_two_stage(users, K, exclude_seen=False)[:2], kept)
    finally:
        s.close()
