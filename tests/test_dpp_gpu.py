"""The DPP calls on the GPU (csrc/dpp.hip behind csrc/serve.hip) against
frecsys_dpp_select, their definition on the host, byte for byte.

test_diversify_dpp_bytes     frecsys_diversify_dpp over the rotated plan of
                             tests/dpp_ref.py: pool sizes on the 64-slot edges
                             up to 1024, k = 1 / pool / a third, (pool, k) on
                             both sides of the factor's LDS / workspace switch,
                             every padded-dim class, 1 / 63 / 65 rows, theta 0 /
                             2 / 8, both relevance modes, Gaussian and grid
                             tables; repeated ids, empty slots, a zero item
                             row, fewer filled slots than k.  Where the factor
                             fits LDS the call runs with it in the workspace
                             too.
test_top_pools_bytes         sorted pools of distinct ids at d = 64: long runs
                             of DPP steps, k = 20 / 64 / 200.
test_recommend_dpp_is_recommend_then_select   USER and EVAL, with and without
                             the history, and a mask that leaves ten.
test_eps_one_is_top_k        eps = 1: frecsys_recommend(k), both arrays.
test_independent             rows permuted, the call split, one MiB of
                             workspace, one item split, gain null.
test_mmr_untouched           recommend_diverse before and after recommend_dpp.
test_bad_arguments           FRECSYS_ERR_INVALID and nothing launched.
"""
import numpy as np
import pytest

import dpp_ref as R
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


@pytest.mark.parametrize("pool,k,dim,rows,m,theta,raw,grid,seed", R.gpu_plan())
def test_diversify_dpp_bytes(monkeypatch, pool, k, dim, rows, m, theta, raw, grid, seed):
    T = R.item_table(m, dim, seed, grid)
    ids, scores = R.random_pools(rows, m, pool, k, seed + 1, grid)
    if raw:  # keep theta * score inside the clamp for most slots
        scores = (scores / np.float32(4.0)).astype(np.float32)
    want = fh.dpp_select(T, ids, scores, k, theta, 1e-3, raw_scores=raw, return_gain=True)
    with _item_ctx(T) as ctx:
        got = ctx.diversify_dpp(ids, scores, k, theta, 1e-3, raw_scores=raw, return_gain=True)
        _same(got, want)
        if R.factor_in_lds(pool, k):  # the same bytes with the factor in the workspace
            monkeypatch.setenv("FRECSYS_DPP_FACTOR", "ws")
            _same(ctx.diversify_dpp(ids, scores, k, theta, 1e-3, raw_scores=raw,
                                    return_gain=True), want)
    filled = (ids >= 0).sum(1)
    assert ((got[0] >= 0).sum(1) == np.minimum(filled, k)).all()


def test_top_pools_bytes():
    """Pools as the scan leaves them (sorted, distinct ids), Gaussian table:
    long runs of DPP steps at d = 64, on both sides of the switch."""
    T, ids, scores = R.gauss_case(64, 9, 700, 200, 9500)
    with _item_ctx(T) as ctx:
        for k, theta in ((20, 4.0), (64, 0.0), (200, 8.0)):
            want = fh.dpp_select(T, ids, scores, k, theta, 1e-3, return_gain=True)
            assert (want[2][:, :min(k, 20)] > 0).all()
            _same(ctx.diversify_dpp(ids, scores, k, theta, 1e-3, return_gain=True), want)


def _serving(seed, dim=64):
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=130, n_items=300)
    rng = np.random.default_rng(seed)
    U = (dim ** -0.25 * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((ni, dim))).astype(np.float32)
    return nu, ni, up, uc, U, V


@pytest.mark.parametrize("side", ("user", "eval"))
def test_recommend_dpp_is_recommend_then_select(side):
    nu, ni, up, uc, U, V = _serving(9501)
    s = fh.SIDE_USER if side == "user" else fh.SIDE_EVAL
    ten = np.zeros(ni, np.uint8)
    ten[[3, 11, 57, 100, 101, 150, 200, 250, 298, 299]] = 1
    with fh.Context(64, nu if side == "user" else 1, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(s, up, uc)
        ctx.set_embeddings(s, U)
        for k, pool, theta, raw, exclude, mask in ((20, 80, 4.0, False, True, None),
                                                   (20, 80, 1.0, True, False, None),
                                                   (7, 33, 0.0, False, False, None),
                                                   (80, 200, 2.0, False, True, None),
                                                   (20, 40, 4.0, False, True, ten)):
            got = ctx.recommend_dpp(s, k, pool, theta, 1e-3, raw_scores=raw,
                                    exclude_history=exclude, item_mask=mask, return_gain=True)
            lists, sc = ctx.recommend(s, pool, exclude_history=exclude, item_mask=mask)
            _same(got, ctx.diversify_dpp(lists, sc, k, theta, 1e-3, raw_scores=raw,
                                         return_gain=True))
            _same(got, fh.dpp_select(V, lists, sc, k, theta, 1e-3, raw_scores=raw,
                                     return_gain=True))
            if mask is not None:  # p < k: the tail is padded
                assert ((got[0] >= 0).sum(1) <= 10).all() and (got[0][:, 10:] == -1).all()
                assert (got[1][:, 10:] == -R.FLT_MAX).all() and (got[2][:, 10:] == -R.FLT_MAX).all()


def test_eps_one_is_top_k():
    """eps = 1 on a normalised table: step 0 takes the most relevant slot, every
    residual drops below 1, and the rest is the fallback in pool order:
    frecsys_recommend(k).  (The rows share a component, so every cosine is
    near 2/3: a residual stays at 1.0f only behind |cos| < 2^-12.5.)"""
    nu, ni, up, uc, U, V = _serving(9502)
    V = V + np.float32(0.5)
    V = (V / np.linalg.norm(V, axis=1, keepdims=True)).astype(np.float32)
    with fh.Context(64, nu, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        for raw in (False, True):
            for k, pool in ((20, 80), (33, 33), (1, 1024)):
                got = ctx.recommend_dpp(fh.SIDE_USER, k, pool, 4.0, 1.0, raw_scores=raw,
                                        return_gain=True)
                _same(got[:2], ctx.recommend(fh.SIDE_USER, k))
                filled = got[0] >= 0  # a user with a long history has fewer than k left
                assert (got[2][:, 0][filled[:, 0]] > 0).all()
                assert (got[2][:, 1:][filled[:, 1:]] == 0).all()


def test_independent(monkeypatch):
    nu, ni, up, uc, U, V = _serving(9503)
    rows = np.random.default_rng(9504).permutation(nu)[:70].astype(np.int64)
    with fh.Context(64, nu, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)

        def run(r, k=20, pool=80, gain=True):
            return ctx.recommend_dpp(fh.SIDE_USER, k, pool, 4.0, 1e-3, rows=r, return_gain=gain)

        base = run(rows)
        perm = np.random.default_rng(9505).permutation(len(rows))
        _same(run(rows[perm]), tuple(a[perm] for a in base))
        halves = [run(rows[:31]), run(rows[31:])]
        _same(tuple(np.concatenate(p) for p in zip(*halves)), base)
        _same(run(rows, gain=False), base[:2])
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", "1")
        _same(run(rows), base)
        monkeypatch.delenv("FRECSYS_RECOMMEND_SPLITS")
        wide = run(rows[:5], 50, 1024)   # the factor in the workspace (204,800 B a row)
        mid = run(rows, 20, 200)         # ... and in LDS (16,000 B)
        lists, sc = ctx.recommend(fh.SIDE_USER, 1024, rows=rows[:5])
        _same(ctx.diversify_dpp(lists, sc, 50, 4.0, 1e-3, return_gain=True), wide)
        _same(ctx.diversify_dpp(lists[:, :200], sc[:, :200], 20, 4.0, 1e-3, return_gain=True),
              tuple(a[:5] for a in run(rows[:5], 20, 200)))
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
        # pool 200: 6 Gramians of 160,000 B fit, so every scan batch takes
        # several sub-batches, and 70 rows at least 12
        ctx.timing_reset()
        _same(run(rows, 20, 200), mid)
        subs = ctx.timing("diversify.gram")[1]
        assert subs == ctx.timing("dpp.select")[1] and subs >= 12
        assert ctx.timing("recommend")[1] >= 2   # explicit row ids over several scan batches
        assert ctx.timing("diversify.select")[1] == 0
        # pool 1024: a Gramian and a factor alone exceed the budget, one row each
        ctx.timing_reset()
        _same(run(rows[:5], 50, 1024), wide)
        assert ctx.timing("diversify.gram")[1] == 5 and ctx.timing("dpp.select")[1] == 5
        ctx.timing_reset()
        _same(ctx.diversify_dpp(lists, sc, 50, 4.0, 1e-3, return_gain=True), wide)
        assert ctx.timing("dpp.select")[1] == 5
        monkeypatch.delenv("FRECSYS_RECOMMEND_WS_MB")
        ctx.timing_reset()
        _same(ctx.diversify_dpp(lists, sc, 50, 4.0, 1e-3, return_gain=True), wide)
        assert ctx.timing("dpp.select")[1] == 1
        flops, nbytes, entities, launches = ctx.work("dpp")
        assert entities == 5 and launches == 1
        assert flops == 5 * (1024 * 1025 * 64 + 50 * 49 * 1024) and nbytes > 0
        # released with the other workspaces, and the bytes stay
        ctx.release_workspaces()
        _same(run(rows), base)


def test_mmr_untouched():
    nu, ni, up, uc, U, V = _serving(9506)
    with fh.Context(64, nu, ni) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        before = ctx.recommend_diverse(fh.SIDE_USER, 20, 80, 0.5, return_mmr=True)
        top = ctx.recommend(fh.SIDE_USER, 20)
        ctx.recommend_dpp(fh.SIDE_USER, 20, 80)
        ctx.recommend_dpp(fh.SIDE_USER, 50, 1024)
        _same(ctx.recommend_diverse(fh.SIDE_USER, 20, 80, 0.5, return_mmr=True), before)
        _same(ctx.recommend(fh.SIDE_USER, 20), top)
        lists, sc = ctx.recommend(fh.SIDE_USER, 80)
        _same(before, fh.mmr_select(V, lists, sc, 20, 0.5, return_mmr=True))


def test_bad_arguments():
    nu, ni, up, uc, U, V = _serving(9700, dim=16)
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

        rd, dv = ctx.recommend_dpp, ctx.diversify_dpp
        invalid(rd, fh.SIDE_USER, 0, 8)
        invalid(rd, fh.SIDE_USER, 9, 8)
        invalid(rd, fh.SIDE_USER, 1, 0)
        invalid(rd, fh.SIDE_USER, 1, 1025)
        invalid(rd, fh.SIDE_USER, 4, 8, -0.1)
        invalid(rd, fh.SIDE_USER, 4, 8, float("inf"))
        invalid(rd, fh.SIDE_USER, 4, 8, float("nan"))
        invalid(rd, fh.SIDE_USER, 4, 8, 4.0, 0.0)
        invalid(rd, fh.SIDE_USER, 4, 8, 4.0, 1.5)
        invalid(rd, fh.SIDE_USER, 4, 8, 4.0, float("nan"))
        invalid(rd, fh.SIDE_ITEM, 4, 8)
        invalid(rd, fh.SIDE_EVAL, 4, 8, rows=[0])          # EVAL never loaded
        invalid(rd, fh.SIDE_USER, 4, 8, rows=[nu])
        invalid(dv, ids, sc, 0)
        invalid(dv, ids, sc, 9)
        invalid(dv, ids, sc, 4, -1.0)
        invalid(dv, ids, sc, 4, 4.0, 0.0)
        invalid(dv, np.full((3, 8), ni, np.int32), sc, 4)
        invalid(dv, ids, np.full((3, 8), np.inf, np.float32), 4)
        wide = sc.copy()
        wide[1, 0], wide[1, 1] = R.FLT_MAX, -R.FLT_MAX
        invalid(dv, ids, wide, 4)
        lib, P = ctx.lib, fh._ptr
        out_i, out_s = np.zeros((3, 4), np.int32), np.zeros((3, 4), np.float32)
        assert lib.frecsys_diversify_dpp(ctx.h, P(ids), P(sc), 3, 8, 4, 4.0, 1e-3, 4, P(out_i),
                                         P(out_s), None) == fh.ERR_INVALID       # unknown flag
        assert lib.frecsys_diversify_dpp(ctx.h, P(ids), P(sc), 3, 8, 4, 4.0, 1e-3, 1, P(out_i),
                                         P(out_s), None) == fh.ERR_INVALID       # not this call's
        assert lib.frecsys_diversify_dpp(ctx.h, P(ids), P(sc), 3, 8, 4, 4.0, 1e-3, 0, None,
                                         P(out_s), None) == fh.ERR_INVALID
        assert lib.frecsys_recommend_dpp(ctx.h, 0, None, 3, 4, 8, 4.0, 1e-3, 8, None, P(out_i),
                                         P(out_s), None) == fh.ERR_INVALID
        assert lib.frecsys_recommend_dpp(ctx.h, 0, None, 3, 4, 8, 4.0, 1e-3, 0, None, None,
                                         P(out_s), None) == fh.ERR_INVALID
        assert lib.frecsys_recommend_dpp(ctx.h, 0, None, 3, 4, 8, 4.0, 1e-3, 0, None, P(out_i),
                                         None, None) == fh.ERR_INVALID
        # zero rows: fine, and nothing is touched
        assert lib.frecsys_diversify_dpp(ctx.h, None, None, 0, 8, 4, 4.0, 1e-3, 0, None, None,
                                         None) == fh.OK
        assert lib.frecsys_recommend_dpp(ctx.h, 0, P(np.zeros(0, np.int64)), 0, 4, 8, 4.0, 1e-3, 0,
                                         None, None, None, None) == fh.OK
        for key in ("recommend", "diversify.gram", "dpp.select"):
            assert ctx.timing(key)[1] == 0, key                                 # nothing launched
        got = rd(fh.SIDE_USER, 4, 8, rows=[0, 0])                              # and it still works
        assert got[0].shape == (2, 4) and (got[0][0] == got[0][1]).all()
