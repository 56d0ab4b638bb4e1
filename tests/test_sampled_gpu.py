"""frecsys_sampled_metrics / frecsys_rank_candidates_metrics on the GPU
(csrc/sampled.hip, then rerank.hip and metrics.hip).  Every comparison is
bitwise: the negatives against the host sampler (itself pinned to the
pure-Python reference by tests/test_sampled_cpu.py), the metrics against
entry points that exist without the feature.

test_device_sampling       neg_count / negatives of the device equal
                           fh.sample_negatives on the CPU grid (items 129 and
                           5000, every n_neg, mask, seed and row mode), 65 and
                           200 rows, USER and EVAL side, three dim classes.
test_sampled_metrics       = list_metrics(rank_candidates(host-built lists)).
test_candidate_metrics     the same composition on caller lists of every
                           length class, ground truth partly / wholly outside
                           the list, masked, in the history.
test_closure               n_neg >= items: every row is a whole-pool row and
                           the result is rank_metrics' bitwise.
test_knob_independent      FRECSYS_RECOMMEND_WS_MB=1: several batches and
                           sub-batches, not a bit changes.
test_user_row_subsets      a USER-side row subset equals the rows of a full call.
test_bad_arguments         FRECSYS_ERR_INVALID before any device call: the
                           timers do not move.
"""
import ctypes

import numpy as np
import pytest

import rerank_ref as Q
import sampled_ref as SR

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

K_DEFAULT = (5, 10, 20, 50, 100)
K_LISTS = (K_DEFAULT, (1024,), (1,))
KEYS = ("sample_negatives", "rank_candidates", "rank_metrics")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tables(m, n_side, dim, seed, gauss=False):
    rng = np.random.default_rng(seed)
    if gauss:
        V = (dim ** -0.25 * rng.standard_normal((m, dim))).astype(np.float32)
        X = (dim ** -0.25 * rng.standard_normal((n_side, dim))).astype(np.float32)
    else:   # integer grid: every score an exact fp32 integer, heavy ties
        V = rng.integers(-2, 3, (m, dim)).astype(np.float32)
        X = rng.integers(-2, 3, (n_side, dim)).astype(np.float32)
    return X, V


def _ctx(side, X, V, ptr, col):
    """A context whose `side` (USER or EVAL) holds X and the histories."""
    ctx = fh.Context(V.shape[1], X.shape[0] if side == fh.SIDE_USER else 1, V.shape[0])
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(side, ptr, col)
    ctx.set_embeddings(side, X)
    return ctx


def _host(m, mask, rows, hist, gp, gi, n_neg, seed):
    return fh.sample_negatives(m, gp, gi, n_neg, seed, rows=rows,
                               hist_ptr=None if hist is None else hist[0],
                               hist_items=None if hist is None else hist[1], item_mask=mask)


def _composed(ctx, side, m, mask, rows, hist, gp, gi, n_neg, k_list, cnt, neg):
    """What a caller composes without the feature: the lists built on the
    host, rank_candidates, list_metrics."""
    cp, ci = SR.lists_from(m, mask, hist, gp, gi, n_neg, cnt, neg)
    items, _ = ctx.rank_candidates(side, max(k_list), cp, ci, rows=rows,
                                   exclude_history=hist is not None, item_mask=mask)
    return fh.list_metrics(items, gp, gi, k_list)


@pytest.mark.parametrize("m,dim,n_rows,side", [
    (129, 20, 65, fh.SIDE_EVAL), (129, 256, 200, fh.SIDE_USER), (129, 1000, 65, fh.SIDE_USER),
    (5000, 20, 200, fh.SIDE_USER), (5000, 256, 65, fh.SIDE_EVAL), (5000, 1000, 200, fh.SIDE_EVAL)])
def test_device_sampling(m, dim, n_rows, side):
    X, V = _tables(m, n_rows, dim, 11 * dim + m)
    plan = SR.plan((m,))
    assert {c[1] for c in plan} == set(SR.GRID_NEG) and {c[2] for c in plan} == set(SR.GRID_MASKS)
    side_csr = SR.histories(n_rows, m, 41)   # one side for every call of the context
    with _ctx(side, X, V, *side_csr) as ctx:
        for _, n_neg, mk, with_hist, seed, row_mode, fseed in plan:
            mask, rows, hist, gp, gi, _ = SR.case(m, n_rows, mk, with_hist, row_mode, fseed,
                                                  side_seed=40)
            cnt, neg = _host(m, mask, rows, hist, gp, gi, n_neg, seed)
            rec, ndcg, dcnt, dneg = ctx.sampled_metrics(
                side, K_DEFAULT, gp, gi, n_neg, seed, rows=rows, exclude_history=with_hist,
                item_mask=mask, return_negatives=True)
            np.testing.assert_array_equal(dcnt, cnt, err_msg=str((n_neg, mk, with_hist)))
            np.testing.assert_array_equal(dneg, neg, err_msg=str((n_neg, mk, with_hist)))
            hrec, hndcg = _composed(ctx, side, m, mask, rows, hist, gp, gi, n_neg, K_DEFAULT,
                                    cnt, neg)
            np.testing.assert_array_equal(_bits(rec), _bits(hrec))
            np.testing.assert_array_equal(_bits(ndcg), _bits(hndcg))


@pytest.mark.parametrize("k_list", K_LISTS)
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("mk", ["none", "m70"])
def test_sampled_metrics(k_list, exclude, mk):
    a = K_LISTS.index(k_list) + 3 * exclude + 6 * (mk == "m70")
    m, dim, n_rows = (5000, 129)[a % 2], (64, 200, 20)[a % 3], 65
    n_neg = (1000, 100, 63, 65)[a % 4] if m == 5000 else (60, 30, 64, 10)[a % 4]
    side = (fh.SIDE_EVAL, fh.SIDE_USER)[(a // 2) % 2]
    X, V = _tables(m, n_rows, dim, 300 + a)
    mask, rows, hist, gp, gi, side_csr = SR.case(m, n_rows, mk, exclude,
                                                 SR.GRID_ROWMODES[a % 3], 300 + a)
    cnt, neg = _host(m, mask, rows, hist, gp, gi, n_neg, 9 + a)
    assert (cnt == n_neg).any()
    with _ctx(side, X, V, *side_csr) as ctx:
        ctx.timing_reset()
        rec, ndcg = ctx.sampled_metrics(side, k_list, gp, gi, n_neg, 9 + a, rows=rows,
                                        exclude_history=exclude, item_mask=mask)
        assert all(ctx.timing(key)[1] >= 1 for key in KEYS)
        lists = int(sum(len(np.unique(gi[gp[i]:gp[i + 1]])) for i in range(n_rows)) + cnt.sum())
        assert ctx.work("rank_candidates")[0] == 2.0 * lists * dim
        assert ctx.work("sample_negatives")[0] == 0.0
        W = 4 * ((m + 127) // 128)
        assert ctx.work("sample_negatives")[1] == 8.0 * W * n_rows + 4.0 * lists
        hrec, hndcg = _composed(ctx, side, m, mask, rows, hist, gp, gi, n_neg, k_list, cnt, neg)
    assert rec.shape == ndcg.shape == (n_rows, len(k_list))
    np.testing.assert_array_equal(_bits(rec), _bits(hrec))
    np.testing.assert_array_equal(_bits(ndcg), _bits(hndcg))
    assert np.isfinite(rec).all() and np.isfinite(ndcg).all()
    assert rec.max() > 0 or max(k_list) == 1   # random scores: a hit at rank 1 is rare


def _candidate_gt(m, cp, ci, ptr, col, mask, exclude, seed):
    """Ground truth per row: ids of the row's own list and ids from anywhere;
    every fourth row only ids that are not in its list; where possible one id
    of the history and one masked-out id."""
    rng = np.random.default_rng(seed)
    off = None if mask is None else np.nonzero(mask == 0)[0]
    gs, kinds = [], set()
    for i in range(len(cp) - 1):
        lst = ci[cp[i]:cp[i + 1]]
        out = np.setdiff1d(np.arange(m), lst)
        g = []
        if i % 4 == 3 and len(out):
            g = list(rng.choice(out, min(len(out), 3), replace=False))
            kinds.add("outside")
        else:
            if len(lst):
                g += list(rng.choice(lst, min(len(lst), 4)))
            if len(out):
                g.append(int(rng.choice(out)))
                if len(lst):
                    kinds.add("partly")
            if not g:
                g = [int(rng.integers(0, m))]
        h = col[ptr[i]:ptr[i + 1]]
        if exclude and len(h) and i % 2 == 0:
            g.append(int(h[0]))
            kinds.add("history")
        if off is not None and len(off) and i % 3 == 1:
            g.append(int(off[i % len(off)]))
            kinds.add("masked")
        gs.append(np.asarray(g, np.int32))
    return SR.csr(gs), kinds


@pytest.mark.parametrize("k_list", K_LISTS)
@pytest.mark.parametrize("m,rows,dim", [(129, 63, 200), (5000, 65, 64)])
def test_candidate_metrics(k_list, m, rows, dim):
    k = max(k_list)
    a = K_LISTS.index(k_list) + (m == 5000)
    exclude, mk = bool(a % 2), ("m70", "none")[(a // 2) % 2]
    X, V, ptr, col, mask, cp, ci = Q.grid_case(m, rows, k, dim, exclude, mk, 5 * a, 8100 + a)
    lens = set(np.diff(cp).tolist())
    assert {0, 1, 63, 65, 1791, 1792, 1793, k - 1, k + 1, 8193, 20000} <= lens
    (gp, gi), kinds = _candidate_gt(m, cp, ci, ptr, col, mask, exclude, 8200 + a)
    assert {"outside", "partly"} <= kinds and ("history" in kinds) == exclude
    assert ("masked" in kinds) == (mask is not None)
    with _ctx(fh.SIDE_EVAL, X, V, ptr, col) as ctx:
        items, _ = ctx.rank_candidates(fh.SIDE_EVAL, k, cp, ci, exclude_history=exclude,
                                       item_mask=mask)
        hrec, hndcg = fh.list_metrics(items, gp, gi, k_list)
        ctx.timing_reset()
        rec, ndcg = ctx.rank_candidates_metrics(fh.SIDE_EVAL, k_list, cp, ci, gp, gi,
                                                exclude_history=exclude, item_mask=mask)
        assert ctx.timing("rank_candidates")[1] == 1 and ctx.timing("rank_metrics")[1] == 1
        assert ctx.timing("sample_negatives")[1] == 0
        assert ctx.work("rank_candidates")[0] == 2.0 * int(cp[-1]) * dim
    np.testing.assert_array_equal(_bits(rec), _bits(hrec))
    np.testing.assert_array_equal(_bits(ndcg), _bits(hndcg))
    assert 0 < (rec > 0).mean() < 1


@pytest.mark.parametrize("m,dim,gauss,exclude,mk", [
    (5000, 64, True, True, "none"), (5000, 200, True, False, "m70"),
    (129, 20, True, True, "m70"), (5000, 20, False, True, "m70"), (129, 256, False, False, "none")])
def test_closure(m, dim, gauss, exclude, mk):
    n_rows = 65
    X, V = _tables(m, n_rows, dim, 500 + dim, gauss)
    mask, rows, hist, gp, gi, side_csr = SR.case(m, n_rows, mk, exclude, "shuffled", 510 + dim)
    with _ctx(fh.SIDE_USER, X, V, *side_csr) as ctx:
        for k_list in (K_DEFAULT, (1024, 1)):
            full = ctx.rank_metrics(fh.SIDE_USER, k_list, gp, gi, rows=rows,
                                    exclude_history=exclude, item_mask=mask)
            for n_neg in (m, m + 77):
                rec, ndcg, cnt, neg = ctx.sampled_metrics(
                    fh.SIDE_USER, k_list, gp, gi, n_neg, 4, rows=rows, exclude_history=exclude,
                    item_mask=mask, return_negatives=True)
                assert (neg == -1).all()
                pools = [len(SR.pool_of(m, mask, [] if hist is None else
                                        hist[1][hist[0][i]:hist[0][i + 1]], gi[gp[i]:gp[i + 1]]))
                         for i in range(n_rows)]
                np.testing.assert_array_equal(cnt, pools)
                np.testing.assert_array_equal(_bits(rec), _bits(full[0]))
                np.testing.assert_array_equal(_bits(ndcg), _bits(full[1]))


def test_knob_independent(monkeypatch):
    m, dim, n_rows, n_neg = 5000, 64, 200, 1000
    X, V = _tables(m, n_rows, dim, 600, True)
    mask, rows, hist, gp, gi, side_csr = SR.case(m, n_rows, "m70", True, "shuffled", 610)
    U = fh.SIDE_USER
    with _ctx(U, X, V, *side_csr) as ctx:
        # per row 640 B of bits, 4 k + 16 B of outputs and about 4 KiB of list.
        # k = 1024: half a MiB holds the fixed part of 110 rows (two batches);
        # k = 10: one batch, whose 800 KiB of ids are cut into sub-batches
        for k_list in ((1024, 10), (10,)):
            ctx.timing_reset()
            base = ctx.sampled_metrics(U, k_list, gp, gi, n_neg, 2, rows=rows, item_mask=mask,
                                       return_negatives=True)
            assert ctx.timing("rank_candidates")[1] == 1   # one batch at the default budget
            lists = SR.lists_from(m, mask, hist, gp, gi, n_neg, base[2], base[3])
            cbase = ctx.rank_candidates_metrics(U, k_list, *lists, gp, gi, rows=rows,
                                                item_mask=mask)
            np.testing.assert_array_equal(_bits(cbase[0]), _bits(base[0]))
            np.testing.assert_array_equal(_bits(cbase[1]), _bits(base[1]))
            monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
            ctx.timing_reset()
            small = ctx.sampled_metrics(U, k_list, gp, gi, n_neg, 2, rows=rows, item_mask=mask,
                                        return_negatives=True)
            assert ctx.timing("rank_candidates")[1] >= 2, "1 MiB must cut 200 rows into batches"
            for x, y in zip(base, small):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
            ctx.timing_reset()
            csmall = ctx.rank_candidates_metrics(U, k_list, *lists, gp, gi, rows=rows,
                                                 item_mask=mask)
            # caller lists: one budget for everything, 8.7 KiB per row at k = 1024
            # (two batches), 4.7 KiB at k = 10 (200 rows just fit)
            assert ctx.timing("rank_candidates")[1] >= (2 if max(k_list) == 1024 else 1)
            np.testing.assert_array_equal(_bits(csmall[0]), _bits(base[0]))
            np.testing.assert_array_equal(_bits(csmall[1]), _bits(base[1]))
            monkeypatch.delenv("FRECSYS_RECOMMEND_WS_MB")
        # the workspaces go with release_workspaces and come back
        before = ctx.counter("live_device_bytes")
        ctx.release_workspaces()
        assert ctx.counter("live_device_bytes") < before
        again = ctx.sampled_metrics(U, k_list, gp, gi, n_neg, 2, rows=rows, item_mask=mask,
                                    return_negatives=True)
        for x, y in zip(base, again):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_user_row_subsets():
    m, dim, nu, n_neg = 5000, 32, 150, 100
    X, V = _tables(m, nu, dim, 700, True)
    mask, _, hist, gp, gi, side_csr = SR.case(m, nu, "none", True, "none", 710)
    with _ctx(fh.SIDE_USER, X, V, *side_csr) as ctx:
        full = ctx.sampled_metrics(fh.SIDE_USER, K_DEFAULT, gp, gi, n_neg, 8,
                                   return_negatives=True)
        rng = np.random.default_rng(711)
        sub = np.concatenate([rng.permutation(nu)[:40], [3, 0, 3]])   # row 3: a whole-pool row
        sp, si = SR.csr([gi[gp[i]:gp[i + 1]] for i in sub])
        part = ctx.sampled_metrics(fh.SIDE_USER, K_DEFAULT, sp, si, n_neg, 8, rows=sub,
                                   return_negatives=True)
        for x, y in zip(full, part):
            np.testing.assert_array_equal(x[sub].view(np.uint32), y.view(np.uint32))
        assert full[2][3] != n_neg and (full[3][3] == -1).all()
        cp, ci = SR.lists_from(m, None, hist, gp, gi, n_neg, full[2], full[3])
        call = ctx.rank_candidates_metrics(fh.SIDE_USER, K_DEFAULT, cp, ci, gp, gi)
        sc = SR.csr([ci[cp[i]:cp[i + 1]] for i in sub])
        cpart = ctx.rank_candidates_metrics(fh.SIDE_USER, K_DEFAULT, sc[0], sc[1], sp, si, rows=sub)
        for x, y in zip(call, cpart):
            np.testing.assert_array_equal(_bits(x[sub]), _bits(y))
        np.testing.assert_array_equal(_bits(call[0]), _bits(full[0]))


def test_bad_arguments():
    m, dim, nu = 40, 16, 50
    X, V = _tables(m, nu, dim, 800, True)
    ptr, col = SR.histories(nu, m, 801)
    gp, gi = np.array([0, 1, 3], np.int64), np.array([1, 2, 3], np.int32)
    cp, ci = np.array([0, 2, 4], np.int64), np.array([1, 5, 2, 6], np.int32)
    with _ctx(fh.SIDE_USER, X, V, ptr, col) as ctx:
        ctx.timing_reset()

        def invalid(fn, *a, **kw):
            with pytest.raises(fh.FrecsysError) as ei:
                fn(*a, **kw)
            assert ei.value.code == fh.ERR_INVALID, ei.value

        sm, cm = ctx.sampled_metrics, ctx.rank_candidates_metrics
        U, rows = fh.SIDE_USER, [0, 1]
        invalid(sm, fh.SIDE_ITEM, [5], gp, gi, 3, rows=rows)
        invalid(sm, U, [5], gp, gi, -1, rows=rows)
        invalid(sm, U, [0], gp, gi, 3, rows=rows)
        invalid(sm, U, [1025], gp, gi, 3, rows=rows)
        invalid(sm, U, [], gp, gi, 3, rows=rows)
        invalid(sm, U, list(range(1, 34)), gp, gi, 3, rows=rows)
        invalid(sm, U, [5], gp, gi, 3, rows=[0, nu])
        invalid(sm, U, [5], gp, gi, 3, rows=[-1, 0])
        invalid(sm, U, [5], [1, 2, 3], gi, 3, rows=rows)              # gt_ptr[0] != 0
        invalid(sm, U, [5], [0, 2, 1], gi, 3, rows=rows)              # not monotone
        invalid(sm, U, [5], [0, 0, 3], gi, 3, rows=rows)              # a row without ground truth
        invalid(sm, U, [5], gp, [1, 2, m], 3, rows=rows)              # id >= n_items
        invalid(sm, U, [5], gp, [1, -2, 3], 3, rows=rows)
        invalid(sm, fh.SIDE_EVAL, [5], gp, gi, 3, rows=rows)          # exclude, EVAL never loaded
        invalid(cm, fh.SIDE_ITEM, [5], cp, ci, gp, gi, rows=rows)
        invalid(cm, U, [0], cp, ci, gp, gi, rows=rows)
        invalid(cm, U, [5], [1, 2, 4], ci, gp, gi, rows=rows)         # cand_ptr[0] != 0
        invalid(cm, U, [5], [0, 3, 2], ci, gp, gi, rows=rows)
        invalid(cm, U, [5], cp, [1, 5, 2, m], gp, gi, rows=rows)
        invalid(cm, U, [5], cp, [1, -1, 2, 6], gp, gi, rows=rows)
        invalid(cm, U, [5], cp, ci, [0, 0, 3], gi, rows=rows)
        invalid(cm, U, [5], cp, ci, gp, [1, 2, m], rows=rows)
        invalid(cm, U, [5], cp, ci, gp, gi, rows=[0, nu])
        # through the C entry points: unknown flag, null pointers, n * n_neg overflow
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ks, out, r2 = np.array([5], np.int32), np.zeros(4, np.float32), np.array([0, 1], np.int64)
        lib = ctx.lib
        S = lambda **kw: lib.frecsys_sampled_metrics(
            ctx.h, 0, P(r2), kw.get("n", 2), kw.get("flags", 0), None, kw.get("gp", P(gp)),
            kw.get("gi", P(gi)), kw.get("n_neg", 3), 1, kw.get("ks", P(ks)), 1,
            kw.get("rec", P(out)), P(out), None, None)
        C = lambda **kw: lib.frecsys_rank_candidates_metrics(
            ctx.h, 0, P(r2), 2, kw.get("cp", P(cp)), kw.get("ci", P(ci)), kw.get("flags", 0), None,
            kw.get("gp", P(gp)), P(gi), kw.get("ks", P(ks)), 1, kw.get("rec", P(out)), P(out))
        for kw in (dict(flags=2), dict(gp=None), dict(gi=None), dict(ks=None), dict(rec=None),
                   dict(n=-1), dict(n=2 ** 62, n_neg=4)):
            assert S(**kw) == fh.ERR_INVALID, kw
        for kw in (dict(flags=2), dict(cp=None), dict(ci=None), dict(gp=None), dict(ks=None),
                   dict(rec=None)):
            assert C(**kw) == fh.ERR_INVALID, kw
        assert all(ctx.timing(key)[1] == 0 for key in KEYS), "a device call before the checks"
        assert S() == fh.OK and C() == fh.OK
        # empty calls touch nothing
        e = ctx.sampled_metrics(U, [5], [0], [], 3, rows=[])
        assert e[0].shape == (0, 1)
        e = ctx.rank_candidates_metrics(U, [5], [0], [], [0], [], rows=[])
        assert e[0].shape == (0, 1)
        # and the context still evaluates: n_neg >= items equals rank_metrics
        a = ctx.sampled_metrics(U, [5, 10], gp, gi, m, 0, rows=rows)
        b = ctx.rank_metrics(U, [5, 10], gp, gi, rows=rows)
        np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))
        np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]))
