"""Model.audience (include/frecsys_model.h) on the ML-1M golden files: iALS at
dim 32 after one epoch.

The model-level lists are bit for bit Context.audience's on the model's own
context, for a thin-query call and for one above the limit; with exclude_seen
no listed user has the item in train.csv; every score is Model.score's of that
(user, item) pair; a user_mask is honoured.  A serve-only load answers without
exclude_seen and refuses it; a model with its tuples answers with exclude_seen
before any train().
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

DIM, K = 32, 20
FLAGS = dict(dim=DIM, stdev=0.1, seed=1, l2_reg=0.003, l2_reg_exp=1.0, uobs_weight=0.1,
             print_train_stats=False)


@pytest.fixture(scope="module")
def model(ml1m):
    """Trained once for the module and closed with it: a model left open would
    keep its context's streams and device memory for the rest of the session."""
    tr, _, _ = ml1m
    m = fh.Model("ials", tr.users, tr.items, **FLAGS)
    m.initialize()
    m.train(1)
    yield m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _seen(tr, n_items):
    """item -> the set of users who have it in the training tuples."""
    seen = [set() for _ in range(n_items)]
    for u, i in zip(np.asarray(tr.users).tolist(), np.asarray(tr.items).tolist()):
        seen[i].add(u)
    return seen


def _items(m, n, seed):
    rng = np.random.default_rng(seed)
    it = np.concatenate([[0, m.n_items - 1], rng.permutation(m.n_items)[:n - 2]])
    it[-1] = it[0]      # a repeated id
    return it.astype(np.int64)


@pytest.mark.parametrize("n", [5, 150])
def test_audience_matches_context_score_and_history(monkeypatch, model, ml1m, n):
    monkeypatch.setenv("FRECSYS_AUDIENCE_THIN_MAX", "64")   # 5: the thin kernel; 150: the scan
    m = model
    ctx = m.context()
    tr, _, _ = ml1m
    thin = fh.audience_plan(DIM, m.n_users, n, K, exclude=True)["thin"]
    assert thin == (1 if n == 5 else 0)
    items = _items(m, n, 21 + n)
    mask = (np.random.default_rng(22).random(m.n_users) < 0.5).astype(np.uint8)
    seen = _seen(tr, m.n_items)
    for exclude, mk in ((True, None), (False, None), (True, mask), (False, mask)):
        users, sc = m.audience(items, K, exclude_seen=exclude, user_mask=mk)
        cu, cs = ctx.audience(K, items=items, exclude_history=exclude, mask=mk)
        assert users.shape == sc.shape == (n, K)
        np.testing.assert_array_equal(users, cu)
        np.testing.assert_array_equal(_bits(sc), _bits(cs))
        assert (users >= 0).all() and np.all(np.diff(sc, axis=1) <= 0)
        np.testing.assert_array_equal(users[-1], users[0])
        if mk is not None:
            assert mk[users].all()
        if exclude:
            for q, it in enumerate(items):
                assert not set(users[q].tolist()) & seen[it], (q, it)
        pair = m.score(users.reshape(-1), np.repeat(items, K).astype(np.int32))
        np.testing.assert_array_equal(_bits(pair), _bits(sc.reshape(-1)))
    # the exclusion matters: a popular item's plain audience holds users who have it
    pop = int(np.argmax([len(s) for s in seen]))
    plain, _ = m.audience([pop], K, exclude_seen=False)
    assert set(plain[0].tolist()) & seen[pop]
    # the default arguments: seen users excluded, no mask
    d_u, d_s = m.audience(items[:3], K)
    e_u, e_s = ctx.audience(K, items=items[:3])
    np.testing.assert_array_equal(d_u, e_u)
    np.testing.assert_array_equal(_bits(d_s), _bits(e_s))


def test_bad_arguments_raise_before_any_device_call(model):
    m = model
    ctx = m.context()
    before = ctx.timing("audience")[1]
    for exclude in (False, True):
        for bad in ([m.n_items], [-1], [0, m.n_items + 5]):
            with pytest.raises(fh.FrecsysError) as ei:
                m.audience(bad, K, exclude_seen=exclude)
            assert ei.value.code == fh.ERR_INVALID
        for k in (0, 1025):
            with pytest.raises(fh.FrecsysError) as ei:
                m.audience([0], k, exclude_seen=exclude)
            assert ei.value.code == fh.ERR_INVALID
    assert ctx.timing("audience")[1] == before
    users, _ = m.audience([], K)
    assert users.shape == (0, K)


def test_serve_only_and_untrained_models(tmp_path, model, ml1m):
    tr, _, _ = ml1m
    items = _items(model, 6, 31)
    want_plain = model.audience(items, K, exclude_seen=False)
    want_excl = model.audience(items, K, exclude_seen=True)
    bare, full = str(tmp_path / "bare.frecsys"), str(tmp_path / "full.frecsys")
    model.save(bare, include_data=False)
    model.save(full)
    b = fh.Model.load(bare)
    try:
        users, sc = b.audience(items, K, exclude_seen=False)
        np.testing.assert_array_equal(users, want_plain[0])
        np.testing.assert_array_equal(_bits(sc), _bits(want_plain[1]))
        with pytest.raises(fh.FrecsysError) as ei:
            b.audience(items, K, exclude_seen=True)
        assert ei.value.code == fh.ERR_INVALID and "serve-only" in str(ei.value)
        users, _ = b.audience(items, K, exclude_seen=False)     # still usable
        np.testing.assert_array_equal(users, want_plain[0])
    finally:
        b.close()
    # loaded with its tuples: the exclusion works before any train()
    f = fh.Model.load(full)
    try:
        users, sc = f.audience(items, K, exclude_seen=True)
        np.testing.assert_array_equal(users, want_excl[0])
        np.testing.assert_array_equal(_bits(sc), _bits(want_excl[1]))
    finally:
        f.close()
    # created from its tuples and never trained: the ITEM CSR is loaded by the call
    g = fh.Model("ials", tr.users, tr.items, **FLAGS)
    try:
        g.initialize()
        seen = _seen(tr, g.n_items)
        users, sc = g.audience(items, K, exclude_seen=True)
        assert (users >= 0).all()
        for q, it in enumerate(items):
            assert not set(users[q].tolist()) & seen[it]
        cu, cs = g.context().audience(K, items=items)
        np.testing.assert_array_equal(users, cu)
        np.testing.assert_array_equal(_bits(sc), _bits(cs))
    finally:
        g.close()
