"""frecsys_rank_candidates / frecsys_score_pairs on the GPU (csrc/rerank.hip)
against the float64 reference of tests/rerank_ref.py and against
frecsys_recommend's own bits.

test_grid_exact                   integer-grid tables: ids equal to rank64 and
                                  score bits equal, no tolerance; every list
                                  length class mixed within one call, repeats,
                                  lists longer than the catalogue.
test_full_list_equals_recommend   each row's list is a permutation of every
                                  id: ids and score BITS equal recommend's.
                                  Decides whether the fmaf chain is the MFMA's.
test_pairs_equal_recommend_scores score_pairs returns recommend's bits per
                                  (row, item), whatever the order or batch.
test_gaussian_float64             Gaussian tables against float64.
test_user_side_row_subsets        USER side, shuffled and repeated row ids.
test_batch_independent            1 MiB row batches: bitwise the same.
test_bad_arguments                FRECSYS_ERR_INVALID, the context still works.
"""
import numpy as np
import pytest

import aux_data as A
import rerank_ref as Q
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
    return np.where(items >= 0, sc, -float(FLT_MAX)).astype(np.float32)


def _gauss(m, rows, dim, seed):
    rng = np.random.default_rng(seed)
    V = (dim ** -0.25 * rng.standard_normal((m, dim))).astype(np.float32)
    X = (dim ** -0.25 * rng.standard_normal((rows, dim))).astype(np.float32)
    return X, V


@pytest.mark.parametrize("m,rows,k,dim,exclude,mk,shift,seed", Q.grid_plan())
def test_grid_exact(m, rows, k, dim, exclude, mk, shift, seed):
    X, V, ptr, col, mask, cp, ci = Q.grid_case(m, rows, k, dim, exclude, mk, shift, seed)
    ref_items, ref_sc = Q.rank64(X, V, ptr, col, None, cp, ci, k, exclude, mask)
    with _eval_ctx(X, V, ptr, col) as ctx:
        items, scores = ctx.rank_candidates(fh.SIDE_EVAL, k, cp, ci, exclude_history=exclude,
                                            item_mask=mask)
    assert items.shape == scores.shape == (rows, k)
    bad = np.nonzero((items != ref_items).any(axis=1))[0]
    assert len(bad) == 0, [(int(r), int(cp[r + 1] - cp[r]), items[r].tolist()[:40],
                            ref_items[r].tolist()[:40]) for r in bad[:2]]
    np.testing.assert_array_equal(_bits(scores), _bits(_expect(ref_items, ref_sc)))
    if mk == "zero":
        assert (items == -1).all()


@pytest.mark.parametrize("m,rows,dim", [(5000, 65, 64), (5000, 65, 500), (1025, 65, 1000)])
def test_full_list_equals_recommend(m, rows, dim):
    X, V = _gauss(m, rows, dim, 91 + dim)
    ptr, col = A.aux_eval(rows, m, 100, 92)
    rng = np.random.default_rng(93)
    ci = np.concatenate([rng.permutation(m) for _ in range(rows)]).astype(np.int32)
    cp = (m * np.arange(rows + 1)).astype(np.int64)
    mask70 = (rng.random(m) < 0.7).astype(np.uint8)
    with _eval_ctx(X, V, ptr, col) as ctx:
        for k in (100, 1024):
            for mask in (None, mask70):
                ri, rs = ctx.recommend(fh.SIDE_EVAL, k, exclude_history=True, item_mask=mask)
                it, sc = ctx.rank_candidates(fh.SIDE_EVAL, k, cp, ci, exclude_history=True,
                                             item_mask=mask)
                diff = _bits(sc) != _bits(rs)
                print(f"full list m={m} dim={dim} k={k} mask={mask is not None}: "
                      f"{int((it != ri).sum())} ids, {int(diff.sum())} score words differ of {it.size}")
                np.testing.assert_array_equal(it, ri)
                np.testing.assert_array_equal(_bits(sc), _bits(rs))


@pytest.mark.parametrize("dim", [20, 256, 1000])
def test_pairs_equal_recommend_scores(dim):
    m, rows = 1000, 65
    X, V = _gauss(m, rows, dim, 95 + dim)
    ptr, col = A.aux_eval(rows, m, 100, 96)
    with _eval_ctx(X, V, ptr, col) as ctx:
        ri, rs = ctx.recommend(fh.SIDE_EVAL, m, exclude_history=False)
        assert (np.sort(ri, axis=1) == np.arange(m)).all()    # every item listed
        S = np.zeros((rows, m), np.float32)
        S[np.arange(rows)[:, None], ri] = rs
        rng = np.random.default_rng(97)
        rr, jj = [a.reshape(-1) for a in np.meshgrid(np.arange(rows), np.arange(m), indexing="ij")]
        rr = np.concatenate([rr, rr[:100], np.full(50, 7)])    # pair, row and item repeats
        jj = np.concatenate([jj, jj[:100], np.full(50, 3)])
        p = rng.permutation(len(rr))
        got = ctx.score_pairs(fh.SIDE_EVAL, rr[p], jj[p])
        diff = _bits(got) != _bits(S[rr[p], jj[p]])
        print(f"pairs dim={dim}: {int(diff.sum())} of {len(p)} score words differ from recommend's")
        np.testing.assert_array_equal(_bits(got), _bits(S[rr[p], jj[p]]))
        assert not np.signbit(got[got == 0]).any()
        p2 = rng.permutation(len(rr))
        got2 = ctx.score_pairs(fh.SIDE_EVAL, rr[p2], jj[p2])
        np.testing.assert_array_equal(_bits(got2), _bits(S[rr[p2], jj[p2]]))
        got7 = ctx.score_pairs(fh.SIDE_EVAL, rr[p][:7], jj[p][:7])
        np.testing.assert_array_equal(_bits(got7), _bits(got[:7]))


@pytest.mark.parametrize("case,list_seed", Q.GAUSS_CASES)
def test_gaussian_float64(case, list_seed):
    m, rows, k, dim, seed = case
    Ue, V, ep, ec, S, _, _ = A.topk_inputs(m, rows, k, dim, seed)
    fin = np.isfinite(S)
    tol = 2e-6 * np.abs(S[fin]).max()
    cp, ci = Q.gauss_lists(m, rows, list_seed)
    ref_items, ref_sc = Q.rank64(Ue, V, ep, ec, None, cp, ci, k + 1, True, None)
    flagged = Q.gauss_flagged(ref_sc, tol)
    assert flagged.sum() <= 0.05 * rows
    ref_items, ref_sc = ref_items[:, :k], ref_sc[:, :k]
    with _eval_ctx(Ue, V, ep, ec) as ctx:
        items, scores = ctx.rank_candidates(fh.SIDE_EVAL, k, cp, ci)
    bad = np.nonzero(~flagged & (items != ref_items).any(axis=1))[0]
    assert len(bad) == 0, [(int(r), items[r].tolist()[:40], ref_items[r].tolist()[:40])
                           for r in bad[:2]]
    listed = items >= 0
    rr = np.broadcast_to(np.arange(rows)[:, None], items.shape)
    S64 = Ue.astype(np.float64) @ V.astype(np.float64).T
    err = np.abs(scores[listed].astype(np.float64) - S64[rr[listed], items[listed]])
    print(f"rank_candidates gaussian m={m} rows={rows} k={k} dim={dim}: "
          f"max score err {err.max(initial=0):.3e} (bar {tol:.3e}), {int(flagged.sum())} rows flagged")
    assert (err <= tol).all()
    assert (scores[~listed] == -FLT_MAX).all()
    np.testing.assert_array_equal(listed.sum(axis=1), (ref_items >= 0).sum(axis=1))
    for r in range(rows):   # nothing from the row's history is listed
        assert not set(items[r][listed[r]].tolist()) & set(ec[ep[r]:ep[r + 1]].tolist())


def test_user_side_row_subsets():
    nu, ni, up, uc, ip, ic = make_quirk_data()
    idle, dim, k = 5, 32, 50
    assert up[idle + 1] == up[idle]
    rng = np.random.default_rng(15)
    U = (dim ** -0.25 * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((ni, dim))).astype(np.float32)

    def lists_for(users):
        out = []
        for u in users:   # half of each list from the row's own history
            h = uc[up[u]:up[u + 1]]
            own = rng.choice(h, min(len(h), 60), replace=False) if len(h) else h[:0]
            out.append(np.concatenate([own, rng.integers(0, ni, 120 - len(own))]).astype(np.int32))
        return (120 * np.arange(len(users) + 1)).astype(np.int64), np.concatenate(out)

    cp, ci = lists_for(range(nu))
    with fh.Context(dim, nu, ni) as ctx:
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        all_i, all_s = ctx.rank_candidates(fh.SIDE_USER, k, cp, ci)
        assert all_i.shape == (nu, k)
        for r in range(nu):
            assert not set(all_i[r].tolist()) & set(uc[up[r]:up[r + 1]].tolist())
        assert (all_i[6] >= 0).sum() <= 60 and (all_i[idle] >= 0).all()
        sub = rng.permutation(nu)[:150]
        sub = np.concatenate([sub, sub[:20], [idle, 6, idle]])   # user 6: 300 items seen
        rng.shuffle(sub)
        scp = np.concatenate([[0], np.cumsum(cp[sub + 1] - cp[sub])]).astype(np.int64)
        sci = np.concatenate([ci[cp[u]:cp[u + 1]] for u in sub])
        it, sc = ctx.rank_candidates(fh.SIDE_USER, k, scp, sci, rows=sub)
        np.testing.assert_array_equal(it, all_i[sub])
        np.testing.assert_array_equal(_bits(sc), _bits(all_s[sub]))
        # without the exclusion the seen candidates come back
        pi, _ = ctx.rank_candidates(fh.SIDE_USER, k, cp[6:8] - cp[6], ci[cp[6]:cp[7]], rows=[6],
                                    exclude_history=False)
        assert set(pi[0].tolist()) & set(uc[up[6]:up[7]].tolist())
    ref_items, _ = Q.rank64(U, V, up, uc, None, cp, ci, k, True, None)
    assert (all_i == ref_items).all(axis=1).mean() > 0.97


def test_batch_independent(monkeypatch):
    m, rows, dim, k, L = 5000, 65, 64, 1024, 8193
    X, V = _gauss(m, rows, dim, 99)
    ptr, col = A.aux_eval(rows, m, k, 98)
    rng = np.random.default_rng(100)
    ci = rng.integers(0, m, rows * L).astype(np.int32)
    cp = (L * np.arange(rows + 1)).astype(np.int64)
    with _eval_ctx(X, V, ptr, col) as ctx:
        ctx.timing_reset()
        base_i, base_s = ctx.rank_candidates(fh.SIDE_EVAL, k, cp, ci)
        assert ctx.timing("rank_candidates")[1] == 1   # one row batch at the default cap
        assert ctx.work("rank_candidates")[0] == 2.0 * rows * L * dim
        ref_items, _ = Q.rank64(X, V, ptr, col, None, cp, ci, k, True, None)
        assert (base_i == ref_items).mean() > 0.99
        # a row's ids (32 KiB), outputs (8 KiB) and history bits (628 B): 25 rows per MiB
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
        ctx.timing_reset()
        it, sc = ctx.rank_candidates(fh.SIDE_EVAL, k, cp, ci)
        assert ctx.timing("rank_candidates")[1] >= 2, "1 MiB must cut 65 rows into batches"
        np.testing.assert_array_equal(it, base_i)
        np.testing.assert_array_equal(_bits(sc), _bits(base_s))
        assert ctx.work("rank_candidates")[0] == 2.0 * rows * L * dim


def test_bad_arguments():
    nu, ni, up, uc, ip, ic = make_quirk_data(n_users=50, n_items=40)
    rng = np.random.default_rng(16)
    U = rng.standard_normal((nu, 16)).astype(np.float32)
    V = rng.standard_normal((ni, 16)).astype(np.float32)
    with fh.Context(16, nu, ni) as ctx:
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.set_embeddings(fh.SIDE_USER, U)
        ctx.set_embeddings(fh.SIDE_ITEM, V)

        def invalid(fn, *a, **kw):
            with pytest.raises(fh.FrecsysError) as ei:
                fn(*a, **kw)
            assert ei.value.code == fh.ERR_INVALID, ei.value

        rk, sp = ctx.rank_candidates, ctx.score_pairs
        invalid(rk, fh.SIDE_USER, 0, [0, 2], [1, 2])
        invalid(rk, fh.SIDE_USER, 1025, [0, 2], [1, 2])
        invalid(rk, fh.SIDE_ITEM, 5, [0, 2], [1, 2], rows=[0])
        invalid(rk, fh.SIDE_USER, 5, [0, 1, 2], [1, 2], rows=[0, nu])
        invalid(rk, fh.SIDE_USER, 5, [0, 2], [1, 2], rows=[-1])
        invalid(rk, fh.SIDE_USER, 5, [1, 2], [1, 2])               # cand_ptr[0] != 0
        invalid(rk, fh.SIDE_USER, 5, [0, 2, 1], [1, 2])            # not monotone
        invalid(rk, fh.SIDE_USER, 5, [0, 2], [1, ni])              # id >= n_items
        invalid(rk, fh.SIDE_USER, 5, [0, 2], [-1, 2])
        invalid(rk, fh.SIDE_EVAL, 5, [0, 2], [1, 2], rows=[0])     # exclude, EVAL never loaded
        invalid(sp, fh.SIDE_ITEM, [0], [0])
        invalid(sp, fh.SIDE_USER, [nu], [0])
        invalid(sp, fh.SIDE_USER, [-1], [0])
        invalid(sp, fh.SIDE_USER, [0], [ni])
        invalid(sp, fh.SIDE_USER, [0], [-1])
        # null pointers, through the C entry points
        import ctypes
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        cp, ci = np.array([0, 2], np.int64), np.array([1, 2], np.int32)
        oi, os_ = np.zeros(5, np.int32), np.zeros(5, np.float32)
        lib = ctx.lib
        assert lib.frecsys_rank_candidates(ctx.h, 0, None, 1, None, P(ci), 5, 0, None, P(oi), P(os_)) == fh.ERR_INVALID
        assert lib.frecsys_rank_candidates(ctx.h, 0, None, 1, P(cp), None, 5, 0, None, P(oi), P(os_)) == fh.ERR_INVALID
        assert lib.frecsys_rank_candidates(ctx.h, 0, None, 1, P(cp), P(ci), 5, 0, None, None, P(os_)) == fh.ERR_INVALID
        assert lib.frecsys_rank_candidates(ctx.h, 0, None, 1, P(cp), P(ci), 5, 2, None, P(oi), P(os_)) == fh.ERR_INVALID
        r1 = np.zeros(1, np.int64)
        assert lib.frecsys_score_pairs(ctx.h, 0, None, P(ci), 1, P(os_)) == fh.ERR_INVALID
        assert lib.frecsys_score_pairs(ctx.h, 0, P(r1), None, 1, P(os_)) == fh.ERR_INVALID
        assert lib.frecsys_score_pairs(ctx.h, 0, P(r1), P(ci), 1, None) == fh.ERR_INVALID
        # scores may be NULL
        assert lib.frecsys_rank_candidates(ctx.h, 0, None, 1, P(cp), P(ci), 5, 0, None, P(oi), None) == fh.OK
        assert set(oi[:2].tolist()) == {1, 2} and (oi[2:] == -1).all()
        # empty calls
        it, sc = ctx.rank_candidates(fh.SIDE_USER, 5, [0], [], rows=[])
        assert it.shape == sc.shape == (0, 5)
        assert ctx.score_pairs(fh.SIDE_USER, [], []).shape == (0,)
        # the context still ranks: user 0 has seen one of the 40 items
        assert up[1] - up[0] == 1
        allc = np.arange(ni, dtype=np.int32)
        it, sc = ctx.rank_candidates(fh.SIDE_USER, 5, [0, ni, 2 * ni], np.concatenate([allc, allc]),
                                     rows=[0, 0])
        ri, rs = ctx.recommend(fh.SIDE_USER, 5, rows=[0, 0])
        np.testing.assert_array_equal(it, ri)
        np.testing.assert_array_equal(_bits(sc), _bits(rs))
        s = ctx.score_pairs(fh.SIDE_USER, [0] * 5, ri[0])
        np.testing.assert_array_equal(_bits(s), _bits(rs[0]))
