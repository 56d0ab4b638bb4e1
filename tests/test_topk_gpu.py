"""Fold-in scoring + top-K on the GPU (csrc/topk.hip, frecsys_eval_topk):
the ranking half of EvaluateDatasetInternal / EvaluateUser
(recommender.h:78-199) against a float64 numpy ranking of the same
embeddings -- history items excluded, scores non-increasing, and the GPU's
k items equal to the exact top k except where scores tie within fp32
rounding of the k-th one.  Exact ties are broken by item id.

test_topk_seams_exact: item counts on the score tile's edge (128 items per
workgroup) and on the tie scan's chunk edge (256 threads), 1 / 63 / 64 / 65
rows (the score tile's 64), k = 1, 33, min(items, 1024), an empty history and
one so long that excluded items are listed.  Every row is the float64 ranking
exactly (numpy_ref.topk64) unless two of its listed scores are within 2e-6
max|S| (test_aux_cpu.test_topk_gap_condition: no more than 5 % of the rows).
"""
import numpy as np
import pytest

import aux_data as A
import numpy_ref as R
import oracle as O
from conftest import make_quirk_data
from test_models_gpu import report
from test_parity_gpu import _ctx

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")


def _ref_topk(Ue, V, ep, ec, k):
    S = Ue.astype(np.float64) @ V.astype(np.float64).T
    for r in range(len(ep) - 1):
        S[r, ec[ep[r]:ep[r + 1]]] = -np.inf
    order = np.lexsort((np.broadcast_to(np.arange(S.shape[1]), S.shape), -S), axis=1)
    return S, order[:, :k]


def _check(top, S, ref, ep, ec, k):
    n = top.shape[0]
    scale = np.abs(S[np.isfinite(S)]).max()
    tol = 2e-6 * scale
    for r in range(n):
        t = top[r]
        assert len(set(t.tolist())) == k
        hist = set(ec[ep[r]:ep[r + 1]].tolist())
        assert not (set(t.tolist()) & hist) or len(hist) + k > S.shape[1]
        st = S[r, t]
        assert np.all(np.diff(st) <= tol), r
        kth = S[r, ref[r, -1]]
        # everything strictly better than the k-th (beyond rounding) is in the list
        must = set(np.where(S[r] > kth + tol)[0].tolist())
        assert must <= set(t.tolist()), r
        assert np.all(st >= kth - tol), r


@pytest.mark.parametrize("dim", [8, 20, 64, 256])
@pytest.mark.parametrize("k", [1, 20, 100])
def test_topk_ml1m_fold_in(ml1m, dim, k):
    tr, vt, ve = ml1m
    nu, ni = tr.max_user + 1, tr.max_item + 1
    up, uc = tr.by_user()
    ip, ic = tr.by_item()
    ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
    ids, ep, ec = vt.compact_users()
    ctx.load_csr(fh.SIDE_EVAL, ep, ec)
    ctx.gramian(fh.SIDE_ITEM)
    ctx.solve_side(fh.SIDE_EVAL, fh.KIND_IALS, 0.003, 0.1)
    Ue = ctx.get_embeddings(fh.SIDE_EVAL)
    top = ctx.eval_topk(k)
    S, ref = _ref_topk(Ue, V, ep, ec, k)
    _check(top, S, ref, ep, ec, k)
    # the lists agree with the exact ranking almost everywhere
    assert np.mean(np.all(top == ref, axis=1)) > 0.97


@pytest.mark.parametrize("dim", [32, 512])
def test_topk_wide_and_large_k(dim):
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=300, n_items=1500)
    ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
    ctx.load_csr(fh.SIDE_EVAL, up, uc)
    ctx.set_embeddings(fh.SIDE_EVAL, U)
    for k in (7, 1024):
        top = ctx.eval_topk(k)
        S, ref = _ref_topk(U, V, up, uc, k)
        _check(top, S, ref, up, uc, k)


def test_topk_ties_by_item_id():
    rng = np.random.default_rng(2)
    nu, ni, dim = 40, 300, 32
    up = np.arange(nu + 1, dtype=np.int64)           # one history item per user
    uc = rng.integers(0, ni, nu).astype(np.int32)
    ctx = fh.Context(dim, nu, ni)
    V = rng.standard_normal((ni, dim)).astype(np.float32)
    V[200:260] = V[5]                                 # 61 identical item rows
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, up, uc)
    Ue = np.tile(V[5], (nu, 1)).astype(np.float32)    # the tied items score highest
    ctx.set_embeddings(fh.SIDE_EVAL, Ue)
    top = ctx.eval_topk(30)
    for r in range(nu):
        tied = [j for j in [5] + list(range(200, 260)) if j != uc[r]]
        assert top[r].tolist() == tied[:30], r


def test_topk_bad_k():
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=50, n_items=40)
    ctx, U, V = _ctx(16, nu, ni, up, uc, ip, ic)
    ctx.load_csr(fh.SIDE_EVAL, up, uc)
    for k in (0, 41, 2000):
        with pytest.raises(fh.FrecsysError) as ei:
            ctx.eval_topk(k)
        assert ei.value.code == fh.ERR_INVALID


def _topk_run(Ue, V, ep, ec, k):
    with fh.Context(V.shape[1], 1, V.shape[0]) as ctx:
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        ctx.load_csr(fh.SIDE_EVAL, ep, ec)
        ctx.set_embeddings(fh.SIDE_EVAL, Ue)
        return ctx.eval_topk(k)


@pytest.mark.parametrize("m,rows,k,dim,seed", A.topk_cases())
def test_topk_seams_exact(m, rows, k, dim, seed):
    Ue, V, ep, ec, S, ref, close = A.topk_inputs(m, rows, k, dim, seed)
    top = _topk_run(Ue, V, ep, ec, k)
    assert top.shape == ref.shape == (rows, k)
    exact = np.all(top == ref, axis=1)
    report(test="aux", entry="eval_topk", items=m, rows=rows, k=k, dim=dim,
           flagged=int(close.sum()), exact_rows=int(exact.sum()))
    assert close.sum() <= 0.05 * rows
    bad = np.nonzero(~exact & ~close)[0]
    assert len(bad) == 0, [(int(r), top[r].tolist(), ref[r].tolist()) for r in bad[:2]]
    for r in np.nonzero(close & ~exact)[0]:
        # scores too close for fp32 to order: the free items by the tolerant
        # check, the excluded ones behind them exactly (ascending id)
        hist = ec[ep[r]:ep[r + 1]]
        kf = min(k, int(np.isfinite(S[r]).sum()))
        np.testing.assert_array_equal(top[r, kf:], ref[r, kf:])
        if kf:
            _check(top[r:r + 1, :kf], np.concatenate([S[r:r + 1], S]), ref[r:r + 1, :kf],
                   np.array([0, len(hist)]), hist, kf)
    if rows > 3:
        # row 3: the k - 1 free items in score order, then the lowest excluded id
        assert exact[3] and not close[3]
        hist = set(ec[ep[3]:ep[4]].tolist())
        assert not (set(top[3, :-1].tolist()) & hist) and top[3, -1] == min(hist)
    if rows > 1:
        assert exact[0] or close[0]  # the empty history


def test_topk_ties_straddle_kth():
    """5 items strictly better than 40 bit-identical rows whose ids fall in
    different chunks of the 256-thread tie scan (1025 items: 5 ids per
    thread), two of them in one chunk; k = 20 takes the 5 in score order and
    the 15 lowest tied ids."""
    rng = np.random.default_rng(12)
    m, dim, rows, k = 1025, 32, 40, 20
    V = rng.standard_normal((m, dim)).astype(np.float32)
    tied = [7, 8] + list(range(33, 33 + 26 * 38, 26))
    better = [1000, 3, 640, 512, 129]  # best first: not in id order
    assert len(tied) == 40 and len({t // 5 for t in tied}) == 39 and not set(tied) & set(better)
    V[tied] = V[7]
    for i, b in enumerate(better):
        V[b] = np.float32(1.5 - 0.1 * i) * V[7]
    Ue = np.tile(V[7], (rows, 1)).astype(np.float32)
    # one history item per row: a better item in rows 0..4, a tied id in 5..19
    uc = rng.integers(0, m, rows).astype(np.int32)
    uc[:5] = better
    uc[5:20] = tied[:30:2]
    ep = np.arange(rows + 1, dtype=np.int64)
    S, ref = R.topk64(Ue, V, ep, uc, k)
    rest = np.setdiff1d(np.arange(m), tied + better)
    assert S[:, rest].max() < S[0, 33] < S[0, 129]
    top = _topk_run(Ue, V, ep, uc, k)
    for r in range(rows):
        want = [j for j in better + tied if j != uc[r]][:k]
        assert top[r].tolist() == want == ref[r].tolist(), r
