"""Model.similar_items / Model.similar_users (include/frecsys_model.h) on the
ML-1M golden files: iALS at dim 32 after one epoch.

The model-level lists are bit for bit Context.similar's on the model's own
context, and satisfy the float64 conditions of tests/similar_ref.check_cosine
against the tables get_embeddings returns.  metric="dot" and include_self map
to the flags; a bad metric string and out-of-range ids raise before any
device call (the "similar" timer's launch count does not move).
"""
import numpy as np
import pytest

import similar_ref as SR

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

DIM, K = 32, 20


@pytest.fixture(scope="module")
def model(ml1m):
    """Trained once for the module and closed with it: a model left open would
    keep its context's streams and device memory for the rest of the session."""
    tr, _, _ = ml1m
    m = fh.Model("ials", tr.users, tr.items, dim=DIM, stdev=0.1, seed=1, l2_reg=0.003,
                 l2_reg_exp=1.0, uobs_weight=0.1, print_train_stats=False)
    m.initialize()
    m.train(1)
    yield m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("side", ["items", "users"])
def test_similar_matches_context_and_float64(model, side):
    m = model
    ctx = m.context()
    cs = fh.SIDE_ITEM if side == "items" else fh.SIDE_USER
    call = m.similar_items if side == "items" else m.similar_users
    n_side = m.n_items if side == "items" else m.n_users
    T = ctx.get_embeddings(cs)
    rng = np.random.default_rng(11)
    rows = np.concatenate([[0, n_side - 1], rng.permutation(n_side)[:200]])
    rows = np.concatenate([rows, rows[:5]])
    mask = (rng.random(n_side) < 0.5).astype(np.uint8)
    tol = SR.cosine_tol(fh.padded_dim(DIM))
    for metric, include_self, mk in (("cosine", False, None), ("cosine", True, mask),
                                     ("dot", False, mask), ("dot", True, None)):
        kw = {("item_mask" if side == "items" else "user_mask"): mk}
        ids, sc = call(rows, K, metric=metric, include_self=include_self, **kw)
        ci, cc = ctx.similar(cs, K, rows=rows, cosine=metric == "cosine", keep_self=include_self,
                             mask=mk)
        assert ids.shape == sc.shape == (len(rows), K)
        np.testing.assert_array_equal(ids, ci)
        np.testing.assert_array_equal(_bits(sc), _bits(cc))
        if not include_self:
            assert (ids != rows[:, None]).all()
        if mk is not None:
            assert mk[ids[ids >= 0]].all()
        if metric == "cosine":
            worst = SR.check_cosine(T, rows, K, include_self, mk, ids, sc, tol)
            print(f"model similar_{side} self={include_self}: max err {worst:.3e} (bar {tol:.3e})")
        else:
            S, _, _ = SR.similar64(T, rows, K, False, include_self, mk)
            listed = ids >= 0
            rr = np.broadcast_to(np.arange(len(rows))[:, None], ids.shape)
            ref = S[rr[listed], ids[listed]]
            assert np.isfinite(ref).all()
            # gamma_Dp of the dot relative to |q||j|
            nrm = np.linalg.norm(T.astype(np.float64), axis=1)
            bound = tol * (nrm[rows][:, None] * nrm[np.where(listed, ids, 0)])[listed]
            assert (np.abs(sc[listed] - ref) <= bound).all()
    # the default arguments: cosine, self excluded, no mask
    d_ids, d_sc = call(rows[:10], K)
    e_ids, e_sc = ctx.similar(cs, K, rows=rows[:10])
    np.testing.assert_array_equal(d_ids, e_ids)
    np.testing.assert_array_equal(_bits(d_sc), _bits(e_sc))


def test_bad_arguments_raise_before_any_device_call(model):
    m = model
    ctx = m.context()
    before = ctx.timing("similar")[1], ctx.timing("similar.norms")[1]
    with pytest.raises(ValueError):
        m.similar_items([0], K, metric="euclid")
    for call, n_side in ((m.similar_items, m.n_items), (m.similar_users, m.n_users)):
        for bad in ([n_side], [-1], [0, n_side + 5]):
            with pytest.raises(fh.FrecsysError) as ei:
                call(bad, K)
            assert ei.value.code == fh.ERR_INVALID
        with pytest.raises(fh.FrecsysError) as ei:
            call([0], 0)
        assert ei.value.code == fh.ERR_INVALID
        with pytest.raises(fh.FrecsysError) as ei:
            call([0], 1025)
        assert ei.value.code == fh.ERR_INVALID
    assert (ctx.timing("similar")[1], ctx.timing("similar.norms")[1]) == before
    ids, _ = m.similar_items([], K)
    assert ids.shape == (0, K)
