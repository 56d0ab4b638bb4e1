"""frecsys_rank_metrics on the GPU (csrc/metrics.hip): Recall@K / NDCG@K
computed on the ranked lists where the fused scoring + top-K left them,
bitwise equal to the host function frecsys_list_metrics applied to
frecsys_recommend's lists -- no tolerance anywhere in this file.

test_device_equals_host     the shapes of tests/test_metrics_cpu.py; exclude
                            on / off, no mask / a 70 % mask; on these exact
                            integer tables also bitwise the CPU oracle.
test_device_equals_host_compacted  5000 items, k = 1024, one item split (the
                            candidate buffers compacted repeatedly).
test_overlapping_ground_truth  ground truth inside the excluded history: no hit.
test_knob_independent       item splits and 1 MiB row batches: the same bits.
test_user_side_rows         shuffled, repeated rows of the USER side; ground
                            truth follows the query position.
test_bad_arguments          FRECSYS_ERR_INVALID, and the context still works.
"""
import itertools

import numpy as np
import pytest

import aux_data as A
import metrics_ref as MR
import oracle as O
import recommend_ref as RR
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref, what):
    (rec, ndcg), (hrec, hndcg) = got, ref
    assert rec.shape == hrec.shape and ndcg.shape == hndcg.shape, what
    bad = np.nonzero((_bits(rec) != _bits(hrec)).any(axis=1) |
                     (_bits(ndcg) != _bits(hndcg)).any(axis=1))[0]
    assert len(bad) == 0, (what, [(int(r), rec[r], hrec[r], ndcg[r], hndcg[r]) for r in bad[:3]])


def _load_eval(ctx, X, ptr, col):
    ctx.load_csr(fh.SIDE_EVAL, ptr, col)
    ctx.set_embeddings(fh.SIDE_EVAL, X)


def _check_case(ctx, X, V, ptr, col, gp, gi, k_list, exclude, mask, oracle):
    K = max(k_list)
    got = ctx.rank_metrics(fh.SIDE_EVAL, k_list, gp, gi, exclude_history=exclude, item_mask=mask)
    items, _ = ctx.recommend(fh.SIDE_EVAL, K, exclude_history=exclude, item_mask=mask)
    host = fh.list_metrics(items, gp, gi, k_list)
    what = (V.shape[0], X.shape[0], k_list, exclude, mask is not None)
    _same(got, host, what)
    if oracle and mask is None:
        zp = np.zeros(len(ptr), np.int64)
        ref = O.evaluate(X, V, ptr if exclude else zp, col, gp, gi, k_list)
        _same(got, ref, ("oracle",) + what)
    return got


@pytest.mark.parametrize("m,rows", list(itertools.product(MR.GRID_M, MR.GRID_ROWS)))
def test_device_equals_host(m, rows):
    cases = [c for c in MR.grid_cases() if c[0] == m and c[1] == rows]
    assert len(cases) >= len(MR.K_LISTS)
    hits = 0
    with fh.Context(MR.GRID_DIM, 1, m) as ctx:
        for _, _, k_list, seed in cases:
            K = max(k_list)
            X, V, ptr, col = RR.grid_inputs(m, rows, K, MR.GRID_DIM, seed)
            gp, gi = MR.ground_truth(rows, m, ptr, col, seed + 5, kmax=min(K, 128))
            ctx.set_embeddings(fh.SIDE_ITEM, V)
            _load_eval(ctx, X, ptr, col)
            for exclude, mk in itertools.product((True, False), ("none", "m70")):
                rec, _ = _check_case(ctx, X, V, ptr, col, gp, gi, k_list, exclude,
                                     RR.grid_mask(m, mk, seed), oracle=True)
                hits += int((rec > 0).sum())
    assert hits > 0 or rows == 1


@pytest.mark.parametrize("exclude,mk", [(True, "m70"), (False, "none")])
def test_device_equals_host_compacted(monkeypatch, exclude, mk):
    m, rows, dim, k_list, seed = 5000, 65, 64, (1024,), 4600
    monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", "1")
    X, V, ptr, col = RR.grid_inputs(m, rows, 1024, dim, seed)
    gp, gi = MR.ground_truth(rows, m, ptr, col, seed + 5, kmax=1024)
    with fh.Context(dim, 1, m) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        _load_eval(ctx, X, ptr, col)
        rec, ndcg = _check_case(ctx, X, V, ptr, col, gp, gi, k_list, exclude,
                                RR.grid_mask(m, mk, seed), oracle=True)
        assert ctx.counter("recommend_splits") == 1
    assert (rec > 0).any() and (ndcg > 0).any()


def test_overlapping_ground_truth():
    m, rows, k_list, seed = 130, 65, (5, 10, 20, 50, 100), 4700
    X, V, ptr, col = RR.grid_inputs(m, rows, 100, MR.GRID_DIM, seed)
    gp, gi = MR.ground_truth(rows, m, ptr, col, seed + 5, disjoint=False)
    over = [set(col[ptr[i]:ptr[i + 1]].tolist()) & set(gi[gp[i]:gp[i + 1]].tolist())
            for i in range(rows)]
    assert sum(bool(o) for o in over) > rows // 2
    with fh.Context(MR.GRID_DIM, 1, m) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        _load_eval(ctx, X, ptr, col)
        got = _check_case(ctx, X, V, ptr, col, gp, gi, k_list, True, None, oracle=False)
        items, _ = ctx.recommend(fh.SIDE_EVAL, 100)
    # an excluded item is never listed, so it is never a hit: the metrics are
    # those of the ground truth without the history items, up to the count g
    for i in range(rows):
        assert not set(items[i].tolist()) & set(col[ptr[i]:ptr[i + 1]].tolist())
    r64, _ = MR.metrics64(items, gp, gi, k_list)
    assert np.abs(got[0] - r64).max() <= np.spacing(np.float32(1.0))


@pytest.mark.parametrize("k_list", [(5, 10, 20, 50, 100), (1024,)])
def test_knob_independent(monkeypatch, k_list):
    m, rows, dim, K = 5000, 130, 64, max(k_list)
    rng = np.random.default_rng(91 + K)
    V = (dim ** -0.25 * rng.standard_normal((m, dim))).astype(np.float32)
    X = (dim ** -0.25 * rng.standard_normal((rows, dim))).astype(np.float32)
    ptr, col = A.aux_eval(rows, m, K, 92)
    gp, gi = MR.ground_truth(rows, m, ptr, col, 93, kmax=K)
    with fh.Context(dim, 1, m) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        _load_eval(ctx, X, ptr, col)
        ctx.timing_reset()
        base = ctx.rank_metrics(fh.SIDE_EVAL, k_list, gp, gi)
        assert ctx.timing("recommend")[1] == 1 and ctx.timing("rank_metrics")[1] == 1
        items, _ = ctx.recommend(fh.SIDE_EVAL, K)
        _same(base, fh.list_metrics(items, gp, gi, k_list), "default")
        assert (base[0] > 0).any()
        for splits in ("1", "3", "7"):
            monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", splits)
            _same(ctx.rank_metrics(fh.SIDE_EVAL, k_list, gp, gi), base, "splits " + splits)
        monkeypatch.delenv("FRECSYS_RECOMMEND_SPLITS")
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
        ctx.timing_reset()
        _same(ctx.rank_metrics(fh.SIDE_EVAL, k_list, gp, gi), base, "1 MiB")
        nb = ctx.timing("rank_metrics")[1]
        assert nb >= 2 and nb == ctx.timing("recommend")[1], "1 MiB must cut 130 rows into batches"
        if K == 1024:
            # one split of 2048 slots of 8 B, the counts, 160 history words, the
            # outputs and the metric row: 25,236 B per row, 41 rows per batch --
            # 41 + 41 + 41 + 7, the last batch partial
            monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", "1")
            ctx.timing_reset()
            _same(ctx.rank_metrics(fh.SIDE_EVAL, k_list, gp, gi), base, "1 MiB, one split")
            assert ctx.timing("rank_metrics")[1] == 4
        flops, nbytes, ents, _ = ctx.work("rank_metrics")
        assert ents % rows == 0 and flops == 2.0 * ents * len(k_list) and nbytes > 0


def test_user_side_rows():
    nu, ni, up, uc, ip, ic = make_quirk_data()
    dim, k_list = 32, (5, 10, 20, 50, 100)
    rng = np.random.default_rng(15)
    U = (dim ** -0.25 * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((ni, dim))).astype(np.float32)
    sub = rng.permutation(nu)[:150]
    gp0, gi0 = MR.ground_truth(sub, ni, up, uc, 16)
    # the first 20 query rows once more at the end, with the same ground truth
    sub = np.concatenate([sub, sub[:20]])
    gp = np.concatenate([gp0, gp0[-1] + gp0[1:21]])
    gi = np.concatenate([gi0, gi0[:gp0[20]]])
    with fh.Context(dim, nu, ni) as ctx:
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        all_items, _ = ctx.recommend(fh.SIDE_USER, 100)
        got = ctx.rank_metrics(fh.SIDE_USER, k_list, gp, gi, rows=sub)
        # ground-truth row i belongs to query position i: the lists of side
        # rows sub[i] against ground-truth rows i
        _same(got, fh.list_metrics(all_items[sub], gp, gi, k_list), "rows=sub")
        _same((got[0][150:], got[1][150:]), (got[0][:20], got[1][:20]), "repeated rows")
        assert (got[0] > 0).any()
        # and not to side row sub[i]: the same ground truth against rows 0 .. 169
        # is another result
        plain = ctx.rank_metrics(fh.SIDE_USER, k_list, gp, gi, rows=np.arange(170))
        _same(plain, fh.list_metrics(all_items[:170], gp, gi, k_list), "rows=0..169")
        assert (_bits(plain[1]) != _bits(got[1])).any()


def test_bad_arguments():
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=50, n_items=40)
    rng = np.random.default_rng(6)
    with fh.Context(16, nu, ni) as ctx:
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, rng.standard_normal((nu, 16)).astype(np.float32))
        ctx.set_embeddings(fh.SIDE_ITEM, rng.standard_normal((ni, 16)).astype(np.float32))

        def invalid(side, k_list, gp, gi, **kw):
            with pytest.raises(fh.FrecsysError) as ei:
                ctx.rank_metrics(side, k_list, gp, gi, **kw)
            assert ei.value.code == fh.ERR_INVALID, ei.value

        invalid(fh.SIDE_USER, (5,), [0, 1, 2], [3, ni], rows=[0, 1])     # id = n_items
        invalid(fh.SIDE_USER, (5,), [0, 0, 2], [3, 4], rows=[0, 1])      # empty row
        invalid(fh.SIDE_USER, (5,), [0, 2, 2], [3, 4], rows=[0, 1])
        invalid(fh.SIDE_ITEM, (5,), [0, 1], [3], rows=[0])
        invalid(fh.SIDE_USER, (5,), [0, 1, 2], [3, 4], rows=[0, nu])
        invalid(fh.SIDE_USER, (5,), [0, 1], [3], rows=[-1])
        invalid(fh.SIDE_USER, (0,), [0, 1], [3], rows=[0])
        invalid(fh.SIDE_USER, (1025,), [0, 1], [3], rows=[0])
        invalid(fh.SIDE_USER, (5,), [0, 1], [-3], rows=[0])
        invalid(fh.SIDE_EVAL, (5,), [0, 1], [3], rows=[0])               # EVAL never loaded
        gp, gi = [0, 2, 3], [3, 39, 7]
        got = ctx.rank_metrics(fh.SIDE_USER, (5, 40), gp, gi, rows=[0, 0])
        items, _ = ctx.recommend(fh.SIDE_USER, 40, rows=[0, 0])
        _same(got, fh.list_metrics(items, gp, gi, (5, 40)), "after errors")
