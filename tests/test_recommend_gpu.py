"""frecsys_recommend on the GPU (csrc/recommend.hip): fused scoring +
streaming top-K with scores, against the float64 reference of
tests/recommend_ref.py.

test_grid_exact          integer-grid tables (every score an exact integer in
                         fp32): ids equal to the reference and scores bitwise
                         equal, no tolerance.  Item counts on the 128-item
                         tile's edges, 1 / 63 / 64 / 65 rows (the 64-row
                         block), k = 1, 33, min(items, 1024) and items + 3,
                         every padded-dim class, history exclusion on / off,
                         no mask / a 70 % mask / an all-zero mask; and with one
                         item split: buffers compacted more than once and the
                         capacity edge of the 2048-slot buffer.
test_gaussian_float64    Gaussian tables (aux_data.topk_inputs): the reference
                         ids on every row the gap condition does not flag,
                         scores within 2e-6 max|S| of float64.
test_split_batch_independent  item splits 1 / 2 / 3 / 7 and 1 MiB row batches:
                         bitwise the same ids and scores.
test_user_side_row_subsets    shuffled, repeated row ids on the USER side.
test_bad_arguments       FRECSYS_ERR_INVALID, and the context still works.
"""
import numpy as np
import pytest

import aux_data as A
import recommend_ref as RR
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

FLT_MAX = np.finfo(np.float32).max


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eval_ctx(X, V, ptr, col):
    ctx = fh.Context(V.shape[1], 1, V.shape[0])
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, ptr, col)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    return ctx


def _expect(items, sc):
    """The reference scores as the library returns them: fp32, -FLT_MAX at -1."""
    return np.where(items >= 0, sc, -float(FLT_MAX)).astype(np.float32)


@pytest.mark.parametrize("m,rows,k,dim,exclude,mk,splits,seed", RR.grid_plan())
def test_grid_exact(monkeypatch, m, rows, k, dim, exclude, mk, splits, seed):
    X, V, ptr, col = RR.grid_inputs(m, rows, k, dim, seed)
    mask = RR.grid_mask(m, mk, seed)
    S, ref_items, ref_sc = RR.recommend64(X, V, ptr, col, None, k, exclude, mask)
    assert np.abs(S[np.isfinite(S)]).max(initial=0) <= 4 * dim
    if splits is not None:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", str(splits))
    with _eval_ctx(X, V, ptr, col) as ctx:
        items, scores = ctx.recommend(fh.SIDE_EVAL, k, exclude_history=exclude, item_mask=mask)
    assert items.shape == scores.shape == (rows, k)
    bad = np.nonzero((items != ref_items).any(axis=1))[0]
    assert len(bad) == 0, [(int(r), items[r].tolist()[:40], ref_items[r].tolist()[:40])
                           for r in bad[:2]]
    np.testing.assert_array_equal(_bits(scores), _bits(_expect(ref_items, ref_sc)))
    if mk == "zero":
        assert (items == -1).all()
    if k > m:
        assert (items[:, m:] == -1).all()
    if exclude and mask is None and rows > 3 and 2 <= k <= m:
        # row 3: k - 1 free items, so the last slot stays empty
        assert items[3, -1] == -1 and items[3, -2] >= 0


def _gauss_cases():
    """One case of aux_data.topk_cases() per item count, the dims rotated."""
    cases = A.topk_cases()
    out = []
    for i, m in enumerate(A.TOPK_M):
        same = [c for c in cases if c[0] == m]
        out.append(same[i % len(same)])
    return out


@pytest.mark.parametrize("m,rows,k,dim,seed", _gauss_cases())
def test_gaussian_float64(m, rows, k, dim, seed):
    Ue, V, ep, ec, _, _, close = A.topk_inputs(m, rows, k, dim, seed)
    S, ref_items, ref_sc = RR.recommend64(Ue, V, ep, ec, None, k, True, None)
    with _eval_ctx(Ue, V, ep, ec) as ctx:
        items, scores = ctx.recommend(fh.SIDE_EVAL, k)
    assert close.sum() <= 0.05 * rows
    ok = ~close
    bad = np.nonzero(ok & (items != ref_items).any(axis=1))[0]
    assert len(bad) == 0, [(int(r), items[r].tolist()[:40], ref_items[r].tolist()[:40])
                           for r in bad[:2]]
    fin = np.isfinite(S)
    tol = 2e-6 * np.abs(S[fin]).max() if fin.any() else 0.0
    listed = items >= 0
    rr = np.broadcast_to(np.arange(rows)[:, None], items.shape)
    err = np.abs(scores[listed].astype(np.float64) - S[rr[listed], items[listed]])
    print(f"recommend gaussian m={m} rows={rows} k={k} dim={dim}: "
          f"max score err {err.max(initial=0):.3e} (bar {tol:.3e})")
    assert np.isfinite(S[rr[listed], items[listed]]).all()
    assert (err <= tol).all()
    assert (scores[~listed] == -FLT_MAX).all()
    # listed counts: every eligible item, up to k
    np.testing.assert_array_equal(listed.sum(axis=1), np.minimum(k, fin.sum(axis=1)))


@pytest.mark.parametrize("k", [100, 1024])
def test_split_batch_independent(monkeypatch, k):
    m, rows, dim = 5000, 65, 64
    rng = np.random.default_rng(77 + k)
    V = (dim ** -0.25 * rng.standard_normal((m, dim))).astype(np.float32)
    X = (dim ** -0.25 * rng.standard_normal((rows, dim))).astype(np.float32)
    ptr, col = A.aux_eval(rows, m, k, 78)
    with _eval_ctx(X, V, ptr, col) as ctx:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", "1")
        ctx.timing_reset()
        base_i, base_s = ctx.recommend(fh.SIDE_EVAL, k)
        assert ctx.timing("recommend")[1] == 1   # one row batch at the default cap
        _, ref_items, _ = RR.recommend64(X, V, ptr, col, None, k, True, None)
        assert (base_i == ref_items).mean() > 0.99  # the sweep itself is sane
        for splits in ("2", "3", "7"):
            monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", splits)
            it, sc = ctx.recommend(fh.SIDE_EVAL, k)
            np.testing.assert_array_equal(it, base_i)
            np.testing.assert_array_equal(_bits(sc), _bits(base_s))
        # 1 MiB of workspace.  The automatic count for 65 rows is one split
        # per 128-item tile within the merge's bound (40 at k = 100, 8 at
        # k = 1024) of 512 / 2048 slots of 8 B: 160 / 128 KiB of candidates
        # per row, at most 8 rows per batch.  One split of 2048 slots (k = 1024) with the row's
        # outputs and history bits is 25 KiB: 41 rows per batch.
        for splits in [None] + (["1"] if k == 1024 else []):
            if splits is None:
                monkeypatch.delenv("FRECSYS_RECOMMEND_SPLITS")
            else:
                monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", splits)
            monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
            ctx.timing_reset()
            it, sc = ctx.recommend(fh.SIDE_EVAL, k)
            assert ctx.timing("recommend")[1] >= 2, "1 MiB must cut 65 rows into batches"
            np.testing.assert_array_equal(it, base_i)
            np.testing.assert_array_equal(_bits(sc), _bits(base_s))
            monkeypatch.delenv("FRECSYS_RECOMMEND_WS_MB")
        flops = ctx.work("recommend")[0]
        assert flops == 2.0 * rows * m * dim


def test_user_side_row_subsets():
    nu, ni, up, uc, ip, ic = make_quirk_data()
    idle, dim, k = 5, 32, 50
    assert up[idle + 1] == up[idle]
    rng = np.random.default_rng(5)
    U = (dim ** -0.25 * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((ni, dim))).astype(np.float32)
    with fh.Context(dim, nu, ni) as ctx:
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        all_i, all_s = ctx.recommend(fh.SIDE_USER, k)
        assert all_i.shape == (nu, k)
        sub = rng.permutation(nu)[:150]
        sub = np.concatenate([sub, sub[:20], [idle, 6, idle]])  # user 6: 300 items seen
        rng.shuffle(sub)
        it, sc = ctx.recommend(fh.SIDE_USER, k, rows=sub)
        np.testing.assert_array_equal(it, all_i[sub])
        np.testing.assert_array_equal(_bits(sc), _bits(all_s[sub]))
        # nothing seen is listed; the idle user gets the plain ranking
        for r in (0, 2, 6, 8):
            assert not set(all_i[r].tolist()) & set(uc[up[r]:up[r + 1]].tolist())
        pi, ps = ctx.recommend(fh.SIDE_USER, k, rows=[idle], exclude_history=False)
        np.testing.assert_array_equal(pi[0], all_i[idle])
        np.testing.assert_array_equal(_bits(ps[0]), _bits(all_s[idle]))
    _, ref_items, _ = RR.recommend64(U, V, up, uc, None, k, True, None)
    assert (all_i == ref_items).all(axis=1).mean() > 0.97


def test_bad_arguments():
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=50, n_items=40)
    rng = np.random.default_rng(6)
    with fh.Context(16, nu, ni) as ctx:
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, rng.standard_normal((nu, 16)).astype(np.float32))
        ctx.set_embeddings(fh.SIDE_ITEM, rng.standard_normal((ni, 16)).astype(np.float32))

        def invalid(*a, **kw):
            with pytest.raises(fh.FrecsysError) as ei:
                ctx.recommend(*a, **kw)
            assert ei.value.code == fh.ERR_INVALID, ei.value

        invalid(fh.SIDE_USER, 0)
        invalid(fh.SIDE_USER, 1025)
        invalid(fh.SIDE_ITEM, 5, rows=[0])
        invalid(fh.SIDE_USER, 5, rows=[0, nu])
        invalid(fh.SIDE_USER, 5, rows=[-1])
        invalid(fh.SIDE_EVAL, 5, rows=[0], exclude_history=True)   # EVAL never loaded
        assert up[1] - up[0] == 1   # user 0 has seen one of the 40 items
        it, sc = ctx.recommend(fh.SIDE_USER, 5, rows=[0, 0])
        assert it.shape == (2, 5) and (it[0] == it[1]).all() and (it >= 0).all()
        assert np.all(np.diff(sc, axis=1) <= 0)
