"""The MMR calls on the GPU (csrc/diversify.hip behind csrc/serve.hip) against
frecsys_mmr_select, their definition on the host, byte for byte.

test_diversify_bytes         frecsys_diversify, by default and with each of
                             FRECSYS_DIVERSIFY_VARIANT = gram / lazy, over the
                             rotated plan of
                             tests/diverse_ref.py: pool sizes on the 32- and
                             64-slot edges up to 1024, k = 1 / pool / a third,
                             every padded-dim class, 1 / 63 / 65 rows, both
                             catalogues, lam 0 / 0.5 / 1, both relevance modes,
                             Gaussian and grid tables; repeated ids, empty
                             slots, a zero item row, fewer filled slots than k.
test_recommend_diverse_is_recommend_then_diversify   USER and EVAL, with and
                             without the history, and a mask that leaves ten.
test_lam_one_is_top_k        lam = 1: frecsys_recommend(k), both arrays.
test_independent             rows permuted, the call split, one row per batch,
                             one item split, mmr null.
test_workspace_owned_and_released   the regions are d_rec's.
test_bad_arguments           FRECSYS_ERR_INVALID and nothing launched.
"""
import numpy as np
import pytest

import diverse_ref as D
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    assert len(got) == len(want)
    np.testing.assert_array_equal(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(_bits(g), _bits(w))


def _item_ctx(T):
    ctx = fh.Context(T.shape[1], 1, T.shape[0])
    ctx.set_embeddings(fh.SIDE_ITEM, T)
    return ctx


@pytest.mark.parametrize("pool,k,dim,rows,m,lam,raw,grid,seed", D.gpu_plan())
def test_diversify_bytes(monkeypatch, pool, k, dim, rows, m, lam, raw, grid, seed):
    T = D.item_table(m, dim, seed, grid)
    ids, scores = D.random_pools(rows, m, pool, k, seed + 1, grid)
    want = fh.mmr_select(T, ids, scores, k, lam, raw_scores=raw, return_mmr=True)
    with _item_ctx(T) as ctx:
        got = ctx.diversify(ids, scores, k, lam, raw_scores=raw, return_mmr=True)
        # both variants: the pool Gramian, and its rows computed per step
        # (a launch per batch: 61 rows of 1023 slots fill the default budget)
        for variant in ("gram", "lazy"):
            monkeypatch.setenv("FRECSYS_DIVERSIFY_VARIANT", variant)
            ctx.timing_reset()
            _same(ctx.diversify(ids, scores, k, lam, raw_scores=raw, return_mmr=True), want)
            selects = ctx.timing("diversify.select")[1]
            assert selects >= 1
            assert ctx.timing("diversify.gram")[1] == (selects if variant == "gram" else 0)
    _same(got, want)
    filled = (ids >= 0).sum(1)
    assert ((got[0] >= 0).sum(1) == np.minimum(filled, k)).all()


def _serving(seed, dim=64):
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=130, n_items=300)
    rng = np.random.default_rng(seed)
    U = (dim ** -0.25 * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((ni, dim))).astype(np.float32)
    return nu, ni, up, uc, U, V


@pytest.mark.parametrize("side", ("user", "eval"))
def test_recommend_diverse_is_recommend_then_diversify(side):
    nu, ni, up, uc, U, V = _serving(8501)
    s = fh.SIDE_USER if side == "user" else fh.SIDE_EVAL
    ten = np.zeros(ni, np.uint8)
    ten[[3, 11, 57, 100, 101, 150, 200, 250, 298, 299]] = 1
    with fh.Context(64, nu if side == "user" else 1, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(s, up, uc)
        ctx.set_embeddings(s, U)
        for k, pool, lam, raw, exclude, mask in ((20, 80, 0.5, False, True, None),
                                                 (20, 80, 0.5, True, False, None),
                                                 (7, 33, 0.2, False, False, None),
                                                 (20, 40, 0.6, False, True, ten)):
            got = ctx.recommend_diverse(s, k, pool, lam, raw_scores=raw, exclude_history=exclude,
                                        item_mask=mask, return_mmr=True)
            lists, sc = ctx.recommend(s, pool, exclude_history=exclude, item_mask=mask)
            _same(got, ctx.diversify(lists, sc, k, lam, raw_scores=raw, return_mmr=True))
            _same(got, fh.mmr_select(V, lists, sc, k, lam, raw_scores=raw, return_mmr=True))
            if mask is not None:  # p < k: the tail is padded
                assert ((got[0] >= 0).sum(1) <= 10).all() and (got[0][:, 10:] == -1).all()
                assert (got[1][:, 10:] == -D.FLT_MAX).all() and (got[2][:, 10:] == -D.FLT_MAX).all()


def test_lam_one_is_top_k():
    nu, ni, up, uc, U, V = _serving(8502)
    with fh.Context(64, nu, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        for raw in (False, True):
            for k, pool in ((20, 80), (33, 33), (1, 1024)):
                got = ctx.recommend_diverse(fh.SIDE_USER, k, pool, 1.0, raw_scores=raw)
                _same(got, ctx.recommend(fh.SIDE_USER, k))


def test_independent(monkeypatch):
    nu, ni, up, uc, U, V = _serving(8503)
    rows = np.random.default_rng(8504).permutation(nu)[:70].astype(np.int64)
    with fh.Context(64, nu, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)

        def run(r, k=20, pool=80, mmr=True):
            return ctx.recommend_diverse(fh.SIDE_USER, k, pool, 0.5, rows=r, return_mmr=mmr)

        base = run(rows)
        perm = np.random.default_rng(8505).permutation(len(rows))
        _same(run(rows[perm]), tuple(a[perm] for a in base))
        halves = [run(rows[:31]), run(rows[31:])]
        _same(tuple(np.concatenate(p) for p in zip(*halves)), base)
        _same(run(rows, mmr=False), base[:2])
        big = run(rows[:5], 50, 1024)
        for variant in ("gram", "lazy"):
            monkeypatch.setenv("FRECSYS_DIVERSIFY_VARIANT", variant)
            _same(run(rows), base)
            _same(run(rows[:5], 50, 1024), big)
        monkeypatch.delenv("FRECSYS_DIVERSIFY_VARIANT")
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", "1")
        _same(run(rows), base)
        monkeypatch.delenv("FRECSYS_RECOMMEND_SPLITS")
        # pool 1024 (300 items: 724 empty slots per row) within 1 MiB: a
        # Gramian alone takes 4 MiB, so every Gramian sub-batch is one row
        wide = run(rows[:5], 50, 1024)
        mid = run(rows, 20, 200)
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
        # pool 200: 6 Gramians of 160,000 B fit, so every scan batch takes
        # several sub-batches, and 70 rows at least 12
        ctx.timing_reset()
        _same(run(rows, 20, 200), mid)
        subs = ctx.timing("diversify.gram")[1]
        assert subs == ctx.timing("diversify.select")[1] and subs >= 12
        assert subs > ctx.timing("recommend")[1] >= 2
        ctx.timing_reset()
        _same(run(rows[:5], 50, 1024), wide)
        assert ctx.timing("diversify.gram")[1] == 5 and ctx.timing("diversify.select")[1] == 5
        assert ctx.timing("recommend")[1] >= 1
        lists, sc = ctx.recommend(fh.SIDE_USER, 1024, rows=rows[:5])
        ctx.timing_reset()
        _same(ctx.diversify(lists, sc, 50, 0.5, return_mmr=True), wide)
        assert ctx.timing("diversify.gram")[1] == 5
        monkeypatch.delenv("FRECSYS_RECOMMEND_WS_MB")
        ctx.timing_reset()
        _same(ctx.diversify(lists, sc, 50, 0.5, return_mmr=True), wide)
        assert ctx.timing("diversify.gram")[1] == 1
        flops, nbytes, entities, launches = ctx.work("diversify")
        assert entities == 5 and launches == 1 and flops > 0 and nbytes > 0


def test_workspace_owned_and_released():
    """The pools, the Gramians and the outputs are regions of the ranking
    workspace: counted by "live_device_bytes", freed by release_workspaces
    (results unchanged afterwards) and with the context."""
    m, dim, n, pool, k = 500, 64, 40, 100, 20
    T = D.gauss_table(m, dim, 8600)
    ids, scores = D.random_pools(n, m, pool, k, 8601, False)
    live = "live_device_bytes"
    with fh.Context(8, 1, 1) as witness:
        b0 = witness.counter(live)
        ctx = _item_ctx(T)
        made = witness.counter(live)
        first = ctx.diversify(ids, scores, k, return_mmr=True)
        held = witness.counter(live)
        assert held - made >= n * (pool * pool * 4 + pool * 8 + k * 12)
        ctx.release_workspaces()
        assert witness.counter(live) == made
        _same(ctx.diversify(ids, scores, k, return_mmr=True), first)
        assert witness.counter(live) == held
        ctx.close()
        assert witness.counter(live) == b0


def test_bad_arguments():
    nu, ni, up, uc, U, V = _serving(8700, dim=16)
    ids = np.zeros((3, 8), np.int32)
    sc = np.zeros((3, 8), np.float32)
    with fh.Context(16, nu, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        ctx.timing_reset()

        def invalid(fn, *a, **kw):
            with pytest.raises(fh.FrecsysError) as ei:
                fn(*a, **kw)
            assert ei.value.code == fh.ERR_INVALID, ei.value

        rd, dv = ctx.recommend_diverse, ctx.diversify
        invalid(rd, fh.SIDE_USER, 0, 8)
        invalid(rd, fh.SIDE_USER, 9, 8)
        invalid(rd, fh.SIDE_USER, 1, 0)
        invalid(rd, fh.SIDE_USER, 1, 1025)
        invalid(rd, fh.SIDE_USER, 4, 8, -0.1)
        invalid(rd, fh.SIDE_USER, 4, 8, 1.5)
        invalid(rd, fh.SIDE_USER, 4, 8, float("nan"))
        invalid(rd, fh.SIDE_ITEM, 4, 8)
        invalid(rd, fh.SIDE_EVAL, 4, 8, rows=[0])          # EVAL never loaded
        invalid(rd, fh.SIDE_USER, 4, 8, rows=[nu])
        invalid(dv, ids, sc, 0)
        invalid(dv, ids, sc, 9)
        invalid(dv, ids, sc, 4, 1.01)
        invalid(dv, np.full((3, 8), ni, np.int32), sc, 4)
        invalid(dv, ids, np.full((3, 8), np.inf, np.float32), 4)
        wide = sc.copy()
        wide[1, 0], wide[1, 1] = D.FLT_MAX, -D.FLT_MAX
        invalid(dv, ids, wide, 4)
        lib, P = ctx.lib, fh._ptr
        out_i, out_s = np.zeros((3, 4), np.int32), np.zeros((3, 4), np.float32)
        assert lib.frecsys_diversify(ctx.h, P(ids), P(sc), 3, 8, 4, 0.5, 4, P(out_i), P(out_s),
                                     None) == fh.ERR_INVALID                     # unknown flag
        assert lib.frecsys_diversify(ctx.h, P(ids), P(sc), 3, 8, 4, 0.5, 1, P(out_i), P(out_s),
                                     None) == fh.ERR_INVALID                     # not diversify's
        assert lib.frecsys_diversify(ctx.h, P(ids), P(sc), 3, 8, 4, 0.5, 0, None, P(out_s),
                                     None) == fh.ERR_INVALID
        assert lib.frecsys_recommend_diverse(ctx.h, 0, None, 3, 4, 8, 0.5, 8, None, P(out_i),
                                             P(out_s), None) == fh.ERR_INVALID
        assert lib.frecsys_recommend_diverse(ctx.h, 0, None, 3, 4, 8, 0.5, 0, None, None, P(out_s),
                                             None) == fh.ERR_INVALID
        assert lib.frecsys_recommend_diverse(ctx.h, 0, None, 3, 4, 8, 0.5, 0, None, P(out_i), None,
                                             None) == fh.ERR_INVALID
        # zero rows: fine, and nothing is touched
        assert lib.frecsys_diversify(ctx.h, None, None, 0, 8, 4, 0.5, 0, None, None, None) == fh.OK
        assert lib.frecsys_recommend_diverse(ctx.h, 0, P(np.zeros(0, np.int64)), 0, 4, 8, 0.5, 0,
                                             None, None, None, None) == fh.OK
        for key in ("recommend", "diversify.gram", "diversify.select"):
            assert ctx.timing(key)[1] == 0, key                                 # nothing launched
        got = rd(fh.SIDE_USER, 4, 8, rows=[0, 0])                              # and it still works
        assert got[0].shape == (2, 4) and (got[0][0] == got[0][1]).all()
