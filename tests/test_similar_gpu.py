"""frecsys_similar on the GPU (csrc/similar.hip, the SIM scan of
csrc/recommend.hip): nearest neighbours inside one factor table, against the
float64 reference of tests/similar_ref.py.

test_dot_exact            integer-grid tables: ids equal to the reference and
                          scores bitwise equal.  Table sizes on the 128-item
                          tile's edges, 1 / 63 / 64 / 65 queries (ids 0, 127,
                          128, m - 1 and a repeated one among them), k = 1, 33,
                          min(m, 1024) and m + 3, four padded-dim classes, no
                          mask / 70 % / all zero, self kept and excluded, both
                          sides, one split and the automatic count; buffers
                          compacted repeatedly and the capacity edges.
test_cosine_exact         +-1 tables (every inverse norm one and the same
                          float, every dot an integer): the ids of the exact
                          dot ranking, the scores bit for bit
                          fl(fl(dot * inv) * inv); zero rows score +0.
test_cosine_float64       Gaussian tables with norms over three decades, within
                          (2 Dp + 8) 2^-24 of float64 -- every row checked.
test_same_chain_as_recommend   similar(dot, keep_self) = recommend with the
                          table on both sides, bit for bit.
test_split_batch_independent   splits 1 / 3 / automatic and 1 MiB row batches.
test_buffers_are_owned_and_released   both buffers counted, freed by
                          release_workspaces and with the context.
test_bad_arguments        FRECSYS_ERR_INVALID, and the tables untouched.
"""
import ctypes

import numpy as np
import pytest

import similar_ref as SR
from recommend_ref import grid_mask

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

FLT_MAX = np.finfo(np.float32).max


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ctx(T, side):
    """A context whose `side` table is T (the other side: one row, unset)."""
    m, dim = T.shape
    ctx = fh.Context(dim, m if side == fh.SIDE_USER else 1, m if side == fh.SIDE_ITEM else 1)
    ctx.set_embeddings(side, T)
    return ctx


def _expect(ids, sc):
    """Reference scores as the library returns them: fp32, -FLT_MAX at -1."""
    return np.where(ids >= 0, sc, -float(FLT_MAX)).astype(np.float32)


def _same_ids(ids, ref_ids):
    bad = np.nonzero((ids != ref_ids).any(axis=1))[0]
    assert len(bad) == 0, [(int(r), ids[r].tolist()[:40], ref_ids[r].tolist()[:40])
                           for r in bad[:2]]


@pytest.mark.parametrize("m,nq,k,dim,mk,keep,side,splits,seed", SR.dot_plan())
def test_dot_exact(monkeypatch, m, nq, k, dim, mk, keep, side, splits, seed):
    assert (SR.USER, SR.ITEM) == (fh.SIDE_USER, fh.SIDE_ITEM)
    T = SR.grid_table(m, dim, seed)
    mask = grid_mask(m, mk, seed)
    rows = SR.query_rows(m, nq, seed)
    S, ref_ids, ref_sc = SR.similar64(T, rows, k, False, keep, mask)
    assert np.abs(S[np.isfinite(S)]).max(initial=0) <= 4 * dim
    if splits is not None:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", str(splits))
    with _ctx(T, side) as ctx:
        ids, scores = ctx.similar(side, k, rows=rows, cosine=False, keep_self=keep, mask=mask)
    assert ids.shape == scores.shape == (len(rows), k)
    _same_ids(ids, ref_ids)
    np.testing.assert_array_equal(_bits(scores), _bits(_expect(ref_ids, ref_sc)))
    if mk == "zero":
        assert (ids == -1).all()
    if not keep:
        assert (ids != rows[:, None]).all()
    if k > m:
        assert (ids[:, m:] == -1).all()


@pytest.mark.parametrize("m,nq,k,dim,mk,keep,side,splits,zeros,seed", SR.cosine_plan())
def test_cosine_exact(monkeypatch, m, nq, k, dim, mk, keep, side, splits, zeros, seed):
    T = SR.sign_table(m, dim, seed, zeros)
    mask = grid_mask(m, mk, seed)
    rows = SR.query_rows(m, nq, seed)
    # the cosine is a strictly increasing function of the integer dot here
    # (one inv for every non-zero row; a zero row has dot 0 and cosine +0
    # with everything), so the ranking is the exact-dot ranking
    _, ref_ids, ref_dot = SR.similar64(T, rows, k, False, keep, mask)
    n2 = (T * T).sum(axis=1, dtype=np.float32)
    assert set(n2.tolist()) <= {0.0, float(dim)}
    inv = np.zeros(m, np.float32)
    inv[n2 > 0] = np.float32(1) / np.sqrt(np.float32(dim))
    listed = ref_ids >= 0
    dot = np.where(listed, ref_dot, 0.0).astype(np.float32)
    want = (dot * inv[rows][:, None]).astype(np.float32) * inv[np.where(listed, ref_ids, 0)]
    want = np.where(listed, want.astype(np.float32) + np.float32(0), -FLT_MAX).astype(np.float32)
    if splits is not None:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", str(splits))
    with _ctx(T, side) as ctx:
        ids, scores = ctx.similar(side, k, rows=rows, cosine=True, keep_self=keep, mask=mask)
    _same_ids(ids, ref_ids)
    np.testing.assert_array_equal(_bits(scores), _bits(want))
    if zeros:
        zq = np.isin(rows, (0, m - 1))                       # zero rows as queries
        zc = listed & np.isin(ids, (0, m - 1))               # and as candidates
        assert zq.any()
        assert (_bits(scores[zq][listed[zq]]) == 0).all()    # +0 bit for bit
        assert (_bits(scores[zc]) == 0).all()


@pytest.mark.parametrize("m,nq,k,dim,mk,keep,side,seed", SR.gauss_plan())
def test_cosine_float64(m, nq, k, dim, mk, keep, side, seed):
    T = SR.gauss_table(m, dim, seed)
    mask = grid_mask(m, mk, seed)
    rows = SR.query_rows(m, nq, seed)
    tol = SR.cosine_tol(fh.padded_dim(dim))
    with _ctx(T, side) as ctx:
        ids, scores = ctx.similar(side, k, rows=rows, cosine=True, keep_self=keep, mask=mask)
        dot_ids, _ = ctx.similar(side, k, rows=rows, cosine=False, keep_self=keep, mask=mask)
    worst = SR.check_cosine(T, rows, k, keep, mask, ids, scores, tol)
    print(f"similar cosine m={m} k={k} dim={dim}: max score err {worst:.3e} (bar {tol:.3e})")
    assert (ids != dot_ids).any()   # the norms matter: the dot ranking is another one
    if keep:
        own = np.ones(len(rows), bool) if mask is None else mask[rows] != 0
        assert ((ids == rows[:, None]).any(axis=1) == own).all()   # cosine 1 is listed


@pytest.mark.parametrize("masked", [False, True])
def test_same_chain_as_recommend(masked):
    m, dim, k = 1025, 200, 50
    T = SR.gauss_table(m, dim, 6200)
    mask = grid_mask(m, "m70", 6200) if masked else None
    with fh.Context(dim, m, m) as ctx:
        ctx.set_embeddings(fh.SIDE_USER, T)
        ctx.set_embeddings(fh.SIDE_ITEM, T)
        ri, rs = ctx.recommend(fh.SIDE_USER, k, exclude_history=False, item_mask=mask)
        for side in (fh.SIDE_ITEM, fh.SIDE_USER):
            si, ss = ctx.similar(side, k, cosine=False, keep_self=True, mask=mask)
            np.testing.assert_array_equal(si, ri)
            np.testing.assert_array_equal(_bits(ss), _bits(rs))
        # the excluding scan computes the same scores: the lists without the query
        xi, xs = ctx.similar(fh.SIDE_ITEM, k, cosine=False, keep_self=False, mask=mask)
        fi, fs = ctx.similar(fh.SIDE_ITEM, k + 1, cosine=False, keep_self=True, mask=mask)
    for r in range(m):
        keep = fi[r] != r
        np.testing.assert_array_equal(xi[r], fi[r][keep][:k])
        np.testing.assert_array_equal(_bits(xs[r]), _bits(fs[r][keep][:k]))


@pytest.mark.parametrize("k", [100, 1024])
@pytest.mark.parametrize("cosine", [False, True])
def test_split_batch_independent(monkeypatch, cosine, k):
    m, nq, dim = 5000, 600, 64
    T = SR.gauss_table(m, dim, 6300 + k)
    rows = SR.query_rows(m, nq, 6301)
    with _ctx(T, fh.SIDE_ITEM) as ctx:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", "1")
        ctx.timing_reset()
        base_i, base_s = ctx.similar(fh.SIDE_ITEM, k, rows=rows, cosine=cosine)
        assert ctx.timing("similar")[1] == 1        # one row batch at the default budget
        assert ctx.timing("similar.norms")[1] == (1 if cosine else 0)
        flops, nbytes = ctx.work("similar")[:2]
        assert flops == 2.0 * nq * m * dim
        assert nbytes == (nq + (2 if cosine else 1) * m) * dim * 4.0 + 8.0 * nq * k
        _, ref_ids, _ = SR.similar64(T, rows, k, cosine, False, None)
        assert (base_i == ref_ids).mean() > 0.99    # the sweep itself is sane
        # 1 MiB of workspace: at one split of 512 / 2048 slots a row takes
        # about 5 / 24 KiB, so 600 rows are at least 3 batches; more splits
        # make more batches
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
        for splits in ("1", "3", None):
            if splits is None:
                monkeypatch.delenv("FRECSYS_RECOMMEND_SPLITS")
            else:
                monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", splits)
            ctx.timing_reset()
            ids, sc = ctx.similar(fh.SIDE_ITEM, k, rows=rows, cosine=cosine)
            assert ctx.timing("similar")[1] >= 2, "1 MiB must cut 600 rows into batches"
            np.testing.assert_array_equal(ids, base_i)
            np.testing.assert_array_equal(_bits(sc), _bits(base_s))


def test_buffers_are_owned_and_released():
    """The candidates workspace and the inverse norms are buffers of the
    context: counted by "live_device_bytes", freed by release_workspaces
    (results unchanged afterwards) and with the context."""
    m, dim, k = 1025, 64, 33
    T = SR.gauss_table(m, dim, 6500)
    live = "live_device_bytes"
    with fh.Context(8, 1, 1) as witness:
        b0 = witness.counter(live)
        ctx = _ctx(T, fh.SIDE_USER)
        made = witness.counter(live)
        ids, sc = ctx.similar(fh.SIDE_USER, k)
        held = witness.counter(live)
        # candidates (one split at least) and outputs per row, and 4 m of norms
        assert held - made >= m * (512 * 8 + k * 8) + 4 * m
        ctx.release_workspaces()
        assert witness.counter(live) == made
        again_i, again_s = ctx.similar(fh.SIDE_USER, k)
        assert witness.counter(live) == held
        np.testing.assert_array_equal(again_i, ids)
        np.testing.assert_array_equal(_bits(again_s), _bits(sc))
        ctx.close()
        assert witness.counter(live) == b0


def test_bad_arguments():
    nu, ni, dim = 50, 40, 16
    rng = np.random.default_rng(6400)
    U = rng.standard_normal((nu, dim)).astype(np.float32)
    V = rng.standard_normal((ni, dim)).astype(np.float32)
    with fh.Context(dim, nu, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_USER, U)

        def invalid(*a, **kw):
            with pytest.raises(fh.FrecsysError) as ei:
                ctx.similar(*a, **kw)
            assert ei.value.code == fh.ERR_INVALID, ei.value

        ctx.set_embeddings(fh.SIDE_ITEM, V)
        # ("a side without embeddings" cannot be reached from here: a context
        # allocates the USER and ITEM tables when it is created, and EVAL, the
        # one side that can lack them, is refused as a side)
        invalid(fh.SIDE_EVAL, 5, rows=[0])
        invalid(7, 5, rows=[0])
        invalid(fh.SIDE_USER, 0)
        invalid(fh.SIDE_USER, 1025)
        invalid(fh.SIDE_ITEM, 5, rows=[0, ni])      # in range for the users only
        invalid(fh.SIDE_USER, 5, rows=[-1])
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ids = np.zeros((nu + 1) * 5, np.int32)
        call = ctx.lib.frecsys_similar
        assert call(ctx.h, fh.SIDE_USER, None, 1, 5, 4, None, P(ids), None) == fh.ERR_INVALID
        assert call(ctx.h, fh.SIDE_USER, None, 1, 5, -1, None, P(ids), None) == fh.ERR_INVALID
        assert call(ctx.h, fh.SIDE_ITEM, None, ni + 1, 5, 0, None, P(ids), None) == fh.ERR_INVALID
        assert call(ctx.h, fh.SIDE_USER, None, 1, 5, 0, None, None, None) == fh.ERR_INVALID
        assert call(ctx.h, fh.SIDE_USER, None, -1, 5, 0, None, P(ids), None) == fh.ERR_INVALID
        assert call(None, fh.SIDE_USER, None, 1, 5, 0, None, P(ids), None) == fh.ERR_INVALID
        # no rows: OK, and nothing is written (not even with null outputs)
        assert call(ctx.h, fh.SIDE_USER, None, 0, 5, 0, None, None, None) == fh.OK
        # scores may be NULL
        assert call(ctx.h, fh.SIDE_USER, None, nu, 5, fh.SIM_COSINE, None, P(ids), None) == fh.OK
        it, sc = ctx.similar(fh.SIDE_USER, 5)
        np.testing.assert_array_equal(ids[:nu * 5].reshape(nu, 5), it)
        assert (it >= 0).all() and (it != np.arange(nu)[:, None]).all()
        assert np.all(np.diff(sc, axis=1) <= 0) and np.abs(sc).max() <= 1.0 + 1e-5
        np.testing.assert_array_equal(ctx.get_embeddings(fh.SIDE_USER), U)
        np.testing.assert_array_equal(ctx.get_embeddings(fh.SIDE_ITEM), V)
