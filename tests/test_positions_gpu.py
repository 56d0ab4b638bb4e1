"""frecsys_rank_positions on the GPU (csrc/positions.hip): the exact position
of every ground-truth item among all eligible items by a fused score-and-count
scan, and mrr / auc per row.  All inputs are exact, so every comparison is an
equality.

test_grid_exact          integer-grid tables (every score an exact integer in
                         fp32): ranks and eligible counts equal to
                         positions_ref.ranks64, mrr / auc bitwise the host
                         function's and the reference's.  The plan covers every
                         pair of: item counts on the 128-item tile's edges,
                         1 / 63 / 64 / 65 rows, four dims, exclusion on / off,
                         no mask / 70 % / all-zero, ground truth of 1, 2,
                         L - 1, L, L + 1 entries (L = the LDS-resident threshold
                         limit) or every item, automatic / 1 / 64 item splits.
test_against_recommend   items <= 1024, k = items, every item ground truth: the
                         place of each listed id in recommend's list is its rank.
test_real_valued         Gaussian tables: the scores of every (row, item) pair
                         from score_pairs (the scan's bits), the words formed and
                         counted in numpy: the device's ranks are equal.  This is
                         the test that catches a scan whose chain differs from
                         the prepared scores.
test_block_mask          whole 64-item half-tiles masked out (two of a block's
                         four waves have nothing to count and run ahead), rows
                         with more than L thresholds: equal to ranks64.
test_split_batch_independent  1 MiB row batches and 1 / 7 / 64 splits: same bytes.
test_user_side_row_subsets    shuffled, repeated rows of the USER side against
                         the EVAL side holding the same vectors.
test_output_subsets      any subset of the four outputs: the same bytes.
test_bad_arguments       FRECSYS_ERR_INVALID by case, nothing written.
"""
import itertools

import numpy as np
import pytest

import aux_data as A
import positions_ref as PR
import recommend_ref as RR
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eval_ctx(X, V, ptr, col):
    ctx = fh.Context(V.shape[1], 1, V.shape[0])
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, ptr, col)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    return ctx


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("m,rows,dim,exclude,mk,gt,splits,seed", PR.plan())
def test_grid_exact(monkeypatch, m, rows, dim, exclude, mk, gt, splits, seed):
    X, V, ptr, col, gp, gi = PR.inputs(m, rows, dim, gt, seed)
    mask = RR.grid_mask(m, mk, seed)
    S, _, _ = RR.recommend64(X, V, ptr, col, None, 1, exclude, mask)
    assert np.abs(S[np.isfinite(S)]).max(initial=0) <= 4 * dim
    ref_rank, ref_elig = PR.ranks64(S, gp, gi)
    if splits is not None:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", str(splits))
    with _eval_ctx(X, V, ptr, col) as ctx:
        rank, elig, mrr, auc = ctx.rank_positions(fh.SIDE_EVAL, gp, gi, exclude_history=exclude,
                                                  item_mask=mask)
        used = ctx.counter("recommend_splits")
        assert ctx.timing("recommend")[1] == 0 and ctx.timing("rank_positions")[1] == 1
    ntiles = (m + 127) // 128
    if splits is not None:
        assert used == min(splits, ntiles)
    bad = np.nonzero(rank != ref_rank)[0]
    assert len(bad) == 0, [(int(t), int(np.searchsorted(gp, t, "right") - 1), int(gi[t]),
                            int(rank[t]), int(ref_rank[t])) for t in bad[:5]]
    np.testing.assert_array_equal(elig, ref_elig)
    hm, ha = fh.position_metrics(rank, gp, elig)
    rm, ra = PR.position_metrics_ref(ref_rank, gp, ref_elig)
    _same((mrr, auc), (hm, ha))
    _same((mrr, auc), (rm, ra))
    if mk == "zero":
        assert (rank == -1).all() and (elig == 0).all() and not mrr.any() and not auc.any()
    if exclude and rows > 1 and PR.gt_count(m, gt) >= 2:
        # row 1's history is {0, m - 1}, and item 0 is in its ground truth
        assert 0 in gi[gp[1]:gp[2]] and (rank[gp[1]:gp[2]][gi[gp[1]:gp[2]] == 0] == -1).all()
    for r in range(4, rows, 5):  # the repeated entry has its first occurrence's rank
        assert rank[gp[r + 1] - 1] == rank[gp[r]]


@pytest.mark.parametrize("m,rows,dim,exclude,mk,seed", [
    (127, 65, 20, True, "none", 61), (1024, 64, 64, True, "m70", 62),
    (1000, 5, 200, False, "m70", 63)])
def test_against_recommend(m, rows, dim, exclude, mk, seed):
    X, V, ptr, col, gp, gi = PR.inputs(m, rows, dim, "all", seed)
    mask = RR.grid_mask(m, mk, seed)
    with _eval_ctx(X, V, ptr, col) as ctx:
        items, _ = ctx.recommend(fh.SIDE_EVAL, m, exclude_history=exclude, item_mask=mask)
        rank, elig = ctx.rank_positions(fh.SIDE_EVAL, gp, gi, exclude_history=exclude,
                                        item_mask=mask, metrics=False)
    np.testing.assert_array_equal(elig, (items >= 0).sum(axis=1))
    for i in range(rows):
        pos = np.full(m, -1, np.int32)
        listed = items[i][items[i] >= 0]
        pos[listed] = np.arange(len(listed), dtype=np.int32)
        np.testing.assert_array_equal(rank[gp[i]:gp[i + 1]], pos[gi[gp[i]:gp[i + 1]]])


def _key(s):
    u = np.ascontiguousarray(s, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint64)


@pytest.mark.parametrize("dim,gt", [(20, "all"), (256, "all"), (256, 10)])
def test_real_valued(dim, gt):
    m, rows = 3000, 65
    rng = np.random.default_rng(90 + dim)
    V = (dim ** -0.25 * rng.standard_normal((m, dim))).astype(np.float32)
    X = (dim ** -0.25 * rng.standard_normal((rows, dim))).astype(np.float32)
    V[7] = V[5]  # exact ties between real scores
    V[2999] = V[5]
    ptr, col = A.aux_eval(rows, m, PR.HIST_K, 91)
    gp, gi = PR.ground_truth(m, rows, gt, ptr, col, 92)
    mask = RR.grid_mask(m, "m70", 93)
    mask[[5, 7, 2999]] = 1
    with _eval_ctx(X, V, ptr, col) as ctx:
        rr = np.repeat(np.arange(rows, dtype=np.int64), m)
        ii = np.tile(np.arange(m, dtype=np.int32), rows)
        sc = ctx.score_pairs(fh.SIDE_EVAL, rr, ii).reshape(rows, m)
        rank, elig, mrr, auc = ctx.rank_positions(fh.SIDE_EVAL, gp, gi, item_mask=mask)
    words = (_key(sc) << np.uint64(32)) | (~np.arange(m, dtype=np.uint32)).astype(np.uint64)
    el = np.broadcast_to(mask != 0, (rows, m)).copy()
    for i in range(rows):
        el[i, col[ptr[i]:ptr[i + 1]]] = False
    ref = np.full(len(gi), -1, np.int32)
    for i in range(rows):
        w = np.sort(words[i][el[i]])  # ascending
        g = gi[gp[i]:gp[i + 1]]
        above = len(w) - np.searchsorted(w, words[i][g], "right")
        ref[gp[i]:gp[i + 1]] = np.where(el[i][g], above, -1)
    bad = np.nonzero(rank != ref)[0]
    assert len(bad) == 0, [(int(t), int(gi[t]), int(rank[t]), int(ref[t])) for t in bad[:5]]
    np.testing.assert_array_equal(elig, el.sum(axis=1))
    _same((mrr, auc), fh.position_metrics(rank, gp, elig))
    assert (rank >= 0).sum() > 0.5 * len(rank) * (gt == "all")


@pytest.mark.parametrize("half,splits", [(0, "1"), (1, "1"), (0, None), (1, "7")])
def test_block_mask(monkeypatch, half, splits):
    """Whole 64-item half-tiles masked out -- the two waves of a row pair that
    own them have nothing to count and run ahead into the next tile while the
    other two still count -- and the other halves masked at random per item,
    so that consecutive tiles have different eligibility words; rows with 1,
    40 (> L: global thresholds) and every item as ground truth in one block,
    a few tiles per split and all of them in one."""
    m, rows, dim = 3000, 65, 64
    X, V, ptr, col = RR.grid_inputs(m, rows, PR.HIST_K, dim, 301 + half)
    parts = [PR.ground_truth(m, rows, kind, ptr, col, 303 + e)
             for e, kind in enumerate(("one", 40, "all"))]
    gp, gi = _interleave(parts, rows)
    ids = np.arange(m)
    mask = (np.random.default_rng(305).random(m) < 0.5).astype(np.uint8)
    mask[(ids % 128) // 64 == half] = 0
    mask[1000:1700] = 0  # and a run of whole tiles
    S, _, _ = RR.recommend64(X, V, ptr, col, None, 1, True, mask)
    ref_rank, ref_elig = PR.ranks64(S, gp, gi)
    if splits is not None:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", splits)
    with _eval_ctx(X, V, ptr, col) as ctx:
        rank, elig, mrr, auc = ctx.rank_positions(fh.SIDE_EVAL, gp, gi, item_mask=mask)
    bad = np.nonzero(rank != ref_rank)[0]
    assert len(bad) == 0, [(int(t), int(gi[t]), int(rank[t]), int(ref_rank[t])) for t in bad[:5]]
    np.testing.assert_array_equal(elig, ref_elig)
    _same((mrr, auc), PR.position_metrics_ref(ref_rank, gp, ref_elig))
    assert (rank >= 0).any() and (rank == -1).any()


def _interleave(parts, rows):
    """Row i of the ground truth parts[i % len(parts)]."""
    pick = [parts[i % len(parts)] for i in range(rows)]
    gi = np.concatenate([p[1][p[0][i]:p[0][i + 1]] for i, p in enumerate(pick)])
    gp = np.concatenate([[0], np.cumsum([p[0][i + 1] - p[0][i]
                                         for i, p in enumerate(pick)])]).astype(np.int64)
    return gp, gi


def test_split_batch_independent(monkeypatch):
    m, rows, dim = 3000, 65, 64
    rng = np.random.default_rng(177)
    V = (dim ** -0.25 * rng.standard_normal((m, dim))).astype(np.float32)
    X = (dim ** -0.25 * rng.standard_normal((rows, dim))).astype(np.float32)
    ptr, col = A.aux_eval(rows, m, PR.HIST_K, 178)
    # rows of 1, 40 and every item: LDS-resident and global thresholds in one block
    parts = [PR.ground_truth(m, rows, kind, ptr, col, 179 + e)
             for e, kind in enumerate(("one", 40, "all"))]
    gp, gi = _interleave(parts, rows)
    with _eval_ctx(X, V, ptr, col) as ctx:
        ctx.timing_reset()
        base = ctx.rank_positions(fh.SIDE_EVAL, gp, gi)
        assert ctx.timing("rank_positions")[1] == 1  # one row batch at the default budget
        assert (base[0] >= 0).any() and (base[0] == -1).any()
        flops, nbytes = ctx.work("rank_positions")[:2]
        assert flops == 2.0 * rows * m * dim
        assert nbytes == 4.0 * len(gi) + 8.0 * (rows + 1) + 4.0 * len(gi) + 12.0 * rows
        for splits in ("1", "7", "64"):
            monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", splits)
            _same(ctx.rank_positions(fh.SIDE_EVAL, gp, gi), base)
            assert ctx.counter("recommend_splits") == min(int(splits), (m + 127) // 128)
        monkeypatch.delenv("FRECSYS_RECOMMEND_SPLITS")
        # 1 MiB: the 22 every-item rows take 3000 * 28 B each, 1.8 MiB, so
        # the 65 rows are cut into two batches at least
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
        ctx.timing_reset()
        _same(ctx.rank_positions(fh.SIDE_EVAL, gp, gi), base)
        assert ctx.timing("rank_positions")[1] >= 2
        assert ctx.timing("recommend")[1] == 0


def test_user_side_row_subsets():
    nu, ni, up, uc, ip, ic = make_quirk_data()
    idle, dim = 5, 32
    rng = np.random.default_rng(5)
    U = (dim ** -0.25 * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((ni, dim))).astype(np.float32)
    sub = rng.permutation(nu)[:150]
    sub = np.concatenate([sub, sub[:20], [idle, 6, idle]])  # user 6: 300 items seen
    rng.shuffle(sub)
    n = len(sub)
    # the subset's histories as a CSR of their own: the EVAL side's below
    hp = np.concatenate([[0], np.cumsum(up[sub + 1] - up[sub])]).astype(np.int64)
    hc = np.concatenate([uc[up[r]:up[r + 1]] for r in sub]).astype(np.int32)
    gp, gi = PR.ground_truth(ni, n, 12, hp, hc, 6)
    with fh.Context(dim, nu, ni) as ctx:
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        got = ctx.rank_positions(fh.SIDE_USER, gp, gi, rows=sub)
        plain = ctx.rank_positions(fh.SIDE_USER, gp, gi, rows=sub, exclude_history=False)
    # the EVAL side holding the same vectors and histories, rows in order
    with _eval_ctx(U[sub], V, hp, hc) as ctx:
        _same(got, ctx.rank_positions(fh.SIDE_EVAL, gp, gi))
        _same(plain, ctx.rank_positions(fh.SIDE_EVAL, gp, gi, exclude_history=False))
    assert (got[0] == -1).any() and (plain[0] >= 0).all()
    assert (plain[1] == ni).all()
    np.testing.assert_array_equal(got[1],
                                  [ni - len(set(uc[up[r]:up[r + 1]].tolist())) for r in sub])


def _raw(ctx, side, rows, n, flags, mask, gp, gi, outs):
    P = fh._ptr
    return ctx.lib.frecsys_rank_positions(ctx.h, side, P(rows), n, flags, P(mask), P(gp), P(gi),
                                          *[P(o) for o in outs])


def test_output_subsets():
    m, rows, dim = 1025, 65, 64
    X, V, ptr, col, gp, gi = PR.inputs(m, rows, dim, "L+1", 71)
    with _eval_ctx(X, V, ptr, col) as ctx:
        full = ctx.rank_positions(fh.SIDE_EVAL, gp, gi)
        _same(ctx.rank_positions(fh.SIDE_EVAL, gp, gi, metrics=False), full[:2])
        for want in itertools.product((False, True), repeat=4):
            outs = [np.full_like(f, 77) if w else None for f, w in zip(full, want)]
            rc = _raw(ctx, fh.SIDE_EVAL, None, rows, fh.REC_EXCLUDE_HISTORY, None, gp, gi, outs)
            if not any(want):
                assert rc == fh.ERR_INVALID
                continue
            assert rc == fh.OK, want
            _same([o for o in outs if o is not None], [f for f, w in zip(full, want) if w])


def test_bad_arguments():
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=50, n_items=40)
    rng = np.random.default_rng(6)
    with fh.Context(16, nu, ni) as ctx:
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, rng.standard_normal((nu, 16)).astype(np.float32))
        ctx.set_embeddings(fh.SIDE_ITEM, rng.standard_normal((ni, 16)).astype(np.float32))
        gp = np.array([0, 2, 3], np.int64)
        gi = np.array([1, 39, 5], np.int32)
        rows = np.array([3, 0], np.int64)
        outs = [np.full(3, 77, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.float32),
                np.full(2, 77, np.float32)]
        EX = fh.REC_EXCLUDE_HISTORY

        def invalid(side=fh.SIDE_USER, r=rows, n=2, flags=EX, mask=None, p=gp, g=gi, o=outs):
            p = None if p is None else np.asarray(p, np.int64)
            g = None if g is None else np.asarray(g, np.int32)
            r = None if r is None else np.asarray(r, np.int64)
            assert _raw(ctx, side, r, n, flags, mask, p, g, o) == fh.ERR_INVALID
            assert b"rank_positions" in ctx.lib.frecsys_last_error(ctx.h)
            assert all((x == 77).all() for x in outs)  # nothing written
            assert ctx.timing("rank_positions")[1] == launches[0]  # no device call

        launches = [0]
        invalid(side=fh.SIDE_ITEM)
        invalid(flags=2)                               # unknown flag
        invalid(n=-1)
        invalid(o=[None] * 4)                          # all four outputs NULL
        invalid(r=[0, nu])                             # row id out of range
        invalid(r=[-1, 0])
        invalid(r=None, n=nu + 1, p=np.arange(nu + 2), g=np.zeros(nu + 1))  # rows > the side's
        invalid(side=fh.SIDE_EVAL)                     # no EVAL embeddings / CSR
        invalid(p=None)
        invalid(p=[1, 2, 3])                           # gt_ptr[0] != 0
        invalid(p=[0, 3, 2])                           # not monotone
        invalid(p=[0, 0, 3])                           # a row with no ground truth
        invalid(g=None)
        invalid(g=[1, -1, 5])
        invalid(g=[1, ni, 5])                          # an id >= n_items
        # a null context: the process's last error, not a context's
        P = fh._ptr
        assert ctx.lib.frecsys_rank_positions(None, fh.SIDE_USER, P(rows), 2, EX, None, P(gp),
                                              P(gi), *[P(o) for o in outs]) == fh.ERR_INVALID
        assert b"rank_positions: null context" in ctx.lib.frecsys_last_error(None)
        assert all((o == 77).all() for o in outs)
        none = np.zeros(1, np.int64)  # no rows: OK, nothing touched
        assert _raw(ctx, fh.SIDE_USER, rows, 0, EX, None, none, None, outs) == fh.OK
        assert all((o == 77).all() for o in outs) and ctx.timing("rank_positions")[1] == 0
        assert _raw(ctx, fh.SIDE_USER, None, 2, EX, None, gp, gi, outs) == fh.OK
        assert ctx.timing("rank_positions")[1] == 1
        assert not any((o == 77).any() for o in outs)  # every output written
        for o in outs:
            o[:] = 77
        launches[0] = 1
        invalid(g=[1, 40, 5])                          # after a good call too
        with pytest.raises(fh.FrecsysError) as ei:
            ctx.rank_positions(fh.SIDE_USER, [0, 1], [40], rows=[0])
        assert ei.value.code == fh.ERR_INVALID
        # and the context still works
        rank, elig, mrr, auc = ctx.rank_positions(fh.SIDE_USER, gp, gi, rows=rows)
        assert (elig == ni - np.array([len(set(uc[up[r]:up[r + 1]].tolist())) for r in rows])).all()
        assert ((rank >= -1) & (rank < ni)).all()
