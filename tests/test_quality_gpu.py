"""The list-quality calls on the GPU (csrc/quality.hip behind csrc/serve.hip)
against frecsys_list_quality, their definition on the host: ILD and novelty
within the bound of include/frecsys_hip.h (tests/quality_ref.py: close),
exposure identical, Recall / NDCG bitwise.

test_lists_quality_matches_host   frecsys_lists_quality on every fixture of
                             tests/quality_ref.py: each padded-dim class, the
                             empty list, one / two slots, one item repeated, the
                             zero row, empty slots in the middle, cut-offs on the
                             64-slot edges and at the K limit, unsorted cut-offs.
test_rank_quality_is_recommend_then_host   pool 0: frecsys_recommend + the host
                             functions; pool > 0: frecsys_recommend_diverse + the
                             same.  USER and EVAL, the exclude flag, a mask that
                             leaves ten items (lists shorter than K).
test_deterministic           ILD / novelty bytes with rows permuted, the call
                             split (exposures add), a 1 MiB workspace, one item
                             split, with and without exposure / ground truth /
                             weights.
test_workspace_owned_and_released   the regions are the ranking workspace's.
test_bad_arguments           FRECSYS_ERR_INVALID and nothing launched.
"""
import numpy as np
import pytest

import quality_ref as Q
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _item_ctx(T):
    ctx = fh.Context(T.shape[1], 1, T.shape[0])
    ctx.set_embeddings(fh.SIDE_ITEM, T)
    return ctx


def _against_host(got, want, what):
    """A device result dict against list_quality's (ild, novelty, exposure)."""
    e_ild = Q.close(got["ild"], want[0])
    e_nov = 0.0 if want[1] is None else Q.close(got["novelty"], want[1])
    print(f"{what}: ild {e_ild:.3f} novelty {e_nov:.3f} of the bound")
    assert e_ild <= 1.0 and e_nov <= 1.0
    assert (got["novelty"] is None) == (want[1] is None)
    np.testing.assert_array_equal(got["exposure"], want[2])


@pytest.mark.parametrize("dim", Q.DIMS)
def test_lists_quality_matches_host(dim):
    T = Q.item_table(Q.M, dim, 9100 + dim)
    L = Q.caller_lists(Q.M, Q.M, 9200 + dim)
    w = Q.item_weights(Q.M, 9300 + dim)
    with _item_ctx(T) as ctx:
        got = ctx.lists_quality(L, Q.K300, w)
        _against_host(got, fh.list_quality(T, L, Q.K300, w), f"dim {dim}")
        assert Q.close(got["ild"], Q.quality64(T, L, Q.K300)[0]) <= 1.0
        uns = ctx.lists_quality(L, Q.K_UNSORTED)
        _against_host(uns, fh.list_quality(T, L, Q.K_UNSORTED), f"dim {dim} unsorted")
        for q, K in enumerate(Q.K_UNSORTED):   # a cut-off's bytes do not depend on its place
            np.testing.assert_array_equal(_bits(uns["ild"][:, q]),
                                          _bits(got["ild"][:, Q.K300.index(K)]))
        assert (got["ild"][0] == 0).all() and (got["ild"][1] == 0).all()
        assert (np.abs(got["ild"][3]) <= Q.BOUND).all() and (got["ild"][8, 1:] == 1).all()
        assert ctx.timing("quality")[1] == 2 and ctx.timing("quality.exposure")[1] == 2


def test_lists_quality_at_the_k_limit():
    T = Q.item_table(Q.M_BIG, Q.DIM_BIG, 9400)
    L = Q.caller_lists(Q.M_BIG, 1024, 9401, rows=10)
    w = Q.item_weights(Q.M_BIG, 9402)
    with _item_ctx(T) as ctx:
        _against_host(ctx.lists_quality(L, Q.K_BIG, w), fh.list_quality(T, L, Q.K_BIG, w), "K 1024")


def _serving(seed, dim=64):
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=130, n_items=300)
    rng = np.random.default_rng(seed)
    U = (dim ** -0.25 * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((ni, dim))).astype(np.float32)
    return nu, ni, up, uc, U, V


def _truth(n, ni, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 9, n)
    gp = np.concatenate([[0], np.cumsum(g)]).astype(np.int64)
    return gp, rng.integers(0, ni, gp[-1]).astype(np.int32)


def _serving_ctx(side, nu, ni, up, uc, U, V):
    s = fh.SIDE_USER if side == "user" else fh.SIDE_EVAL
    ctx = fh.Context(V.shape[1], nu if side == "user" else 1, ni)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(s, up, uc)
    ctx.set_embeddings(s, U)
    return s, ctx


@pytest.mark.parametrize("side", ("user", "eval"))
def test_rank_quality_is_recommend_then_host(side):
    nu, ni, up, uc, U, V = _serving(9501)
    w = Q.item_weights(ni, 9502)
    gt = _truth(nu, ni, 9503)
    ten = np.zeros(ni, np.uint8)
    ten[[3, 11, 57, 100, 101, 150, 200, 250, 298, 299]] = 1
    ks = (1, 5, 20, 64)
    s, ctx = _serving_ctx(side, nu, ni, up, uc, U, V)
    with ctx:
        for pool, lam, raw, exclude, mask in ((None, 0.7, False, True, None),
                                              (None, 0.7, False, False, ten),
                                              (200, 0.5, False, True, None),
                                              (64, 0.3, True, False, None),
                                              (100, 0.6, False, True, ten)):
            got = ctx.rank_quality(s, ks, pool=pool, lam=lam, raw_scores=raw, item_weight=w,
                                   gt=gt, exclude_history=exclude, item_mask=mask)
            if pool is None:
                lists = ctx.recommend(s, max(ks), exclude_history=exclude, item_mask=mask)[0]
            else:
                lists = ctx.recommend_diverse(s, max(ks), pool, lam, raw_scores=raw,
                                              exclude_history=exclude, item_mask=mask)[0]
            _against_host(got, fh.list_quality(V, lists, ks, w), f"{side} pool {pool}")
            rec, ndcg = fh.list_metrics(lists, gt[0], gt[1], ks)
            np.testing.assert_array_equal(_bits(got["recall"]), _bits(rec))
            np.testing.assert_array_equal(_bits(got["ndcg"]), _bits(ndcg))
            if mask is not None:   # ten eligible items: the lists are shorter than 20 and 64
                assert (got["exposure"].sum(1) <= 10 * nu).all()
                assert got["exposure"][:, ten == 0].sum() == 0
                np.testing.assert_array_equal(_bits(got["ild"][:, 2]), _bits(got["ild"][:, 3]))


def test_deterministic(monkeypatch):
    nu, ni, up, uc, U, V = _serving(9601)
    w = Q.item_weights(ni, 9602)
    rows = np.random.default_rng(9603).permutation(nu)[:70].astype(np.int64)
    ks = (3, 20, 64)
    s, ctx = _serving_ctx("user", nu, ni, up, uc, U, V)
    with ctx:
        def run(r, pool=200, **kw):
            kw.setdefault("item_weight", w)
            return ctx.rank_quality(s, ks, rows=r, pool=pool, lam=0.5, **kw)

        def same(got, want, sel=slice(None)):
            for key in ("ild", "novelty"):
                np.testing.assert_array_equal(_bits(got[key]), _bits(want[key][sel]))

        for pool in (None, 200):
            base = run(rows, pool, gt=_truth(len(rows), ni, 9604))
            perm = np.random.default_rng(9605).permutation(len(rows))
            p = run(rows[perm], pool)
            same(p, base, perm)
            np.testing.assert_array_equal(p["exposure"], base["exposure"])
            a, b = run(rows[:31], pool), run(rows[31:], pool)
            same(a, base, slice(0, 31))
            same(b, base, slice(31, None))
            np.testing.assert_array_equal(a["exposure"] + b["exposure"], base["exposure"])
            # fewer outputs: the others keep their bytes
            no_ex = run(rows, pool, exposure=False)
            assert no_ex["exposure"] is None and no_ex["recall"] is None
            same(no_ex, base)
            no_w = run(rows, pool, item_weight=None)
            assert no_w["novelty"] is None
            np.testing.assert_array_equal(_bits(no_w["ild"]), _bits(base["ild"]))
            only_nov = run(rows, pool, ild=False, exposure=False)
            assert only_nov["ild"] is None
            np.testing.assert_array_equal(_bits(only_nov["novelty"]), _bits(base["novelty"]))
            only_ex = run(rows, pool, ild=False, item_weight=None)
            np.testing.assert_array_equal(only_ex["exposure"], base["exposure"])
            monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", "1")
            same(run(rows, pool), base)
            monkeypatch.delenv("FRECSYS_RECOMMEND_SPLITS")
            monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
            # the rows three times over: 210 rows take several 64-row batches of 1 MiB
            gp, gi = _truth(len(rows), ni, 9604)
            gp3 = np.concatenate([[0]] + [gp[1:] + t * gp[-1] for t in range(3)])
            thrice = np.tile(np.arange(len(rows)), 3)
            ctx.timing_reset()
            small = run(rows[thrice], pool, gt=(gp3, np.tile(gi, 3)))
            assert ctx.timing("recommend")[1] >= 2
            assert ctx.timing("quality")[1] == ctx.timing("recommend")[1]
            assert ctx.timing("quality.exposure")[1] == ctx.timing("recommend")[1]
            same(small, base, thrice)
            np.testing.assert_array_equal(small["exposure"], 3 * base["exposure"])
            np.testing.assert_array_equal(_bits(small["recall"]), _bits(base["recall"][thrice]))
            np.testing.assert_array_equal(_bits(small["ndcg"]), _bits(base["ndcg"][thrice]))
            monkeypatch.delenv("FRECSYS_RECOMMEND_WS_MB")
        # caller lists: one row per batch against all rows at once
        lists = ctx.recommend(s, 64, rows=rows)[0]
        whole = ctx.lists_quality(lists, ks, w)
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
        wide = np.full((len(rows), 300000), -1, np.int32)   # 1.2 MB a row: one row per batch
        wide[:, :64] = lists
        ctx.timing_reset()
        one = ctx.lists_quality(wide, ks, w)
        assert ctx.timing("quality")[1] == len(rows)
        same(one, whole)
        np.testing.assert_array_equal(one["exposure"], whole["exposure"])
        flops, nbytes, entities, launches = ctx.work("quality")
        assert entities > 0 and flops > 0 and nbytes > 0


def test_workspace_owned_and_released():
    T = Q.item_table(Q.M, 64, 9700)
    L = Q.caller_lists(Q.M, Q.M, 9701)
    w = Q.item_weights(Q.M, 9702)
    live = "live_device_bytes"
    with fh.Context(8, 1, 1) as witness:
        b0 = witness.counter(live)
        ctx = _item_ctx(T)
        made = witness.counter(live)
        first = ctx.lists_quality(L, Q.K300, w)
        held = witness.counter(live)
        # the lists, the result rows, the weights and the counts
        assert held - made >= L.size * 4 + L.shape[0] * 6 * 8 + Q.M * 4 + 6 * Q.M * 8
        ctx.release_workspaces()
        assert witness.counter(live) == made
        again = ctx.lists_quality(L, Q.K300, w)
        for key in ("ild", "novelty"):
            np.testing.assert_array_equal(_bits(again[key]), _bits(first[key]))
        np.testing.assert_array_equal(again["exposure"], first["exposure"])
        assert witness.counter(live) == held
        ctx.close()
        assert witness.counter(live) == b0


def test_bad_arguments():
    nu, ni, up, uc, U, V = _serving(9800, dim=16)
    w = Q.item_weights(ni, 9801)
    gt = _truth(nu, ni, 9802)
    s, ctx = _serving_ctx("user", nu, ni, up, uc, U, V)
    with ctx:
        ctx.timing_reset()

        def invalid(fn, *a, **kw):
            with pytest.raises(fh.FrecsysError) as ei:
                fn(*a, **kw)
            assert ei.value.code == fh.ERR_INVALID, ei.value
            return str(ei.value)

        rq, lq = ctx.rank_quality, ctx.lists_quality
        assert "cut-offs must be in [1, 1024]" in invalid(rq, s, (0, 5))
        assert "cut-offs must be in [1, 1024]" in invalid(rq, s, (5, 1025))
        assert "k_list must hold 1 to 32 cut-offs" in invalid(rq, s, ())
        assert "k_list must hold 1 to 32 cut-offs" in invalid(rq, s, (1,) * 33)
        assert "every output is null" in invalid(rq, s, (5,), ild=False, exposure=False)
        bad = w.copy()
        bad[7] = np.nan
        assert "item_weight[7] is not finite" in invalid(rq, s, (5,), item_weight=bad)
        assert "pool must be in [1, 1024]" in invalid(rq, s, (5,), pool=1025)
        assert "pool must be in [1, 1024]" in invalid(rq, s, (5,), pool=-1)
        assert "k must be in [1, pool]" in invalid(rq, s, (5, 9), pool=8)
        assert "lam must be in [0, 1]" in invalid(rq, s, (5,), pool=8, lam=1.5)
        assert "lam must be in [0, 1]" in invalid(rq, s, (5,), pool=8, lam=float("nan"))
        assert "div_flags without a pool" in invalid(rq, s, (5,), raw_scores=True)
        assert "side must be USER or EVAL" in invalid(rq, fh.SIDE_ITEM, (5,))
        assert "out of range" in invalid(rq, s, (5,), rows=[nu])
        short = (gt[0][:-1].copy(), gt[1])
        short[0][3] = short[0][2]                               # a row with no ground truth
        assert "has no ground truth" in invalid(rq, s, (5,), rows=np.arange(nu - 1), gt=short)
        over = (gt[0], np.where(np.arange(len(gt[1])) == 4, ni, gt[1]).astype(np.int32))
        assert "ground-truth id" in invalid(rq, s, (5,), gt=over)
        assert "cut-offs must be in [1, 8]" in invalid(lq, np.zeros((2, 8), np.int32), (9,))
        assert f"item id {ni} out of range" in invalid(lq, np.full((2, 8), ni, np.int32), (8,))
        lib, P = ctx.lib, fh._ptr
        k1 = np.array([5], np.int32)
        out = np.zeros((nu, 1), np.float32)
        ex = np.ones((1, ni), np.int64)

        def raw(flags=1, weight=None, gp=None, gi=None, ild=out, nov=None, rec=None, ndcg=None,
                n=nu, div_flags=0, pool=0, exposure=None):
            return lib.frecsys_rank_quality(ctx.h, 0, None, n, flags, None, P(k1), 1, pool, 0.5,
                                            div_flags, P(weight), P(gp), P(gi), P(ild), P(nov),
                                            P(rec), P(ndcg), P(exposure))

        assert raw() == fh.OK
        ctx.timing_reset()
        assert raw(flags=2) == fh.ERR_INVALID                                   # unknown flag
        assert raw(div_flags=1, pool=8) == fh.ERR_INVALID                       # not a div flag
        assert raw(weight=w) == fh.ERR_INVALID                                  # weights, no novelty
        assert raw(nov=out) == fh.ERR_INVALID                                   # novelty, no weights
        assert raw(rec=out, ndcg=out) == fh.ERR_INVALID                         # no ground truth
        assert raw(gp=gt[0], gi=gt[1], rec=out) == fh.ERR_INVALID               # ndcg missing
        assert raw(n=-1) == fh.ERR_INVALID
        # zero rows: fine, nothing touched but the exposure, which is zeroed
        assert raw(n=0, exposure=ex) == fh.OK and (ex == 0).all()
        ex[:] = 1
        assert lib.frecsys_lists_quality(ctx.h, None, 0, 8, P(k1), 1, None, None, None,
                                         P(ex)) == fh.OK and (ex == 0).all()
        for key in ("recommend", "diversify.select", "rank_metrics", "quality",
                    "quality.exposure"):
            assert ctx.timing(key)[1] == 0, key                                 # nothing launched
        got = rq(s, (5,), rows=[0, 0])                                          # and it still works
        assert (got["ild"][0] == got["ild"][1]).all() and got["exposure"].sum() == 10
