"""frecsys_audience on the GPU (csrc/audience.hip, and the scan of
csrc/recommend.hip above the thin-query limit): the k best users for items,
against the float64 reference of tests/audience_ref.py.  Every kernel seam
(chunk rows, queries per pass, slots) comes from fh.audience_plan.

test_grid_exact           integer-grid tables: ids equal to the reference and
                          score bits equal, no tolerance.  Users around one
                          and two chunks, queries around one and two passes,
                          six dims, k = 1, 33, min(m, 1024), m + 3, mask none /
                          70 % / all zero, exclusion on / off with the rows of
                          aux_data.aux_eval as the ITEM CSR, a query id twice
                          in one pass, an all-zero user row and an all-zero
                          query (+0 bits); with one split the capacity edges
                          of the smallest and the largest buffer and buffers
                          compacted more than once.
test_thin_equals_scan     every grid case on the scan path
                          (FRECSYS_AUDIENCE_THIN_MAX=0) and 63 / 64 / 65
                          queries on both paths: identical ids and score bits.
test_split_pass_batch_independent   splits 1 / 3 / 7 / automatic, 1 MiB batches.
test_gaussian_float64     Gaussian tables within 2e-6 max|S| of float64.
test_same_bits_as_score_pairs_and_recommend   one chain, three calls.
test_item_row_subsets     shuffled and repeated item ids, the exclusion.
test_bad_arguments        FRECSYS_ERR_INVALID, and a good call afterwards.
test_buffers_are_owned_and_released   the workspace is the context's.
"""
import ctypes

import numpy as np
import pytest

import audience_ref as AR
import aux_data as A
from conftest import make_quirk_data
from recommend_ref import grid_mask

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

FLT_MAX = np.finfo(np.float32).max
THIN = "FRECSYS_AUDIENCE_THIN_MAX"


def _plan(dim, m, n, k, **kw):
    return fh.audience_plan(dim, m, n, k, **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ctx(V, U, iptr=None, icol=None):
    """A context with the item table V, the user table U and (if given) the
    ITEM-side CSR."""
    ctx = fh.Context(V.shape[1], U.shape[0], V.shape[0])
    ctx.set_embeddings(fh.SIDE_USER, U)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    if iptr is not None:
        ctx.load_csr(fh.SIDE_ITEM, iptr, icol)
    return ctx


def _expect(ids, sc):
    """The reference scores as the library returns them: fp32, -FLT_MAX at -1."""
    return np.where(ids >= 0, sc, -float(FLT_MAX)).astype(np.float32)


def _same_ids(ids, ref_ids):
    bad = np.nonzero((ids != ref_ids).any(axis=1))[0]
    assert len(bad) == 0, [(int(r), ids[r].tolist()[:40], ref_ids[r].tolist()[:40])
                           for r in bad[:2]]


def _grid(monkeypatch, m, n, k, dim, exclude, mk, splits, seed):
    """The case's inputs, reference and context, the splits knob set."""
    V, U, iptr, icol, items = AR.grid_case(m, n, k, dim, seed)
    mask = grid_mask(m, mk, seed)
    S, ref_ids, ref_sc = AR.audience64(V, U, iptr, icol, items, k, exclude, mask)
    assert np.abs(S[np.isfinite(S)]).max(initial=0) <= 4 * dim
    if splits is not None:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", str(splits))
    return V, U, items, mask, ref_ids, ref_sc, _ctx(V, U, iptr, icol)


_GRID = []


def _case(i):
    """Case i of audience_ref.grid_plan.  The plan is asked when the first test
    runs, not when the module is collected: collecting loads no library."""
    if not _GRID:
        _GRID.extend(AR.grid_plan(_plan))
        assert len(_GRID) == AR.GRID_CASES
    return _GRID[i]


@pytest.mark.parametrize("case", range(AR.GRID_CASES))
def test_grid_exact(monkeypatch, case):
    m, n, k, dim, exclude, mk, splits, seed = _case(case)
    assert _plan(dim, m, n, k)["thin"] == 1
    V, U, items, mask, ref_ids, ref_sc, ctx = _grid(monkeypatch, m, n, k, dim, exclude, mk,
                                                    splits, seed)
    with ctx:
        ids, scores = ctx.audience(k, items=items, exclude_history=exclude, mask=mask)
    assert ids.shape == scores.shape == (n, k)
    _same_ids(ids, ref_ids)
    np.testing.assert_array_equal(_bits(scores), _bits(_expect(ref_ids, ref_sc)))
    if mk == "zero":
        assert (ids == -1).all()
    if k > m:
        assert (ids[:, m:] == -1).all()
    if n >= 5:      # item 1 twice in the first pass
        np.testing.assert_array_equal(ids[4], ids[1])
    listed = ids >= 0
    if n >= 6:      # the all-zero query: +0, not the -0 of a product-first chain
        assert (_bits(scores[5][listed[5]]) == 0).all()
    if m >= 2:      # the all-zero user row
        assert (_bits(scores[listed & (ids == m // 2)]) == 0).all()
    if exclude and mask is None and n >= 4 and 2 <= k <= m:
        # item 3: k - 1 users free, so the last slot stays empty
        assert ids[3, -1] == -1 and ids[3, -2] >= 0


@pytest.mark.parametrize("case", range(AR.GRID_CASES))
def test_thin_equals_scan(monkeypatch, case):
    m, n, k, dim, exclude, mk, splits, seed = _case(case)
    V, U, items, mask, ref_ids, _, ctx = _grid(monkeypatch, m, n, k, dim, exclude, mk, splits,
                                               seed)
    with ctx:
        ti, ts = ctx.audience(k, items=items, exclude_history=exclude, mask=mask)
        monkeypatch.setenv(THIN, "0")
        assert _plan(dim, m, n, k)["thin"] == 0
        si, ss = ctx.audience(k, items=items, exclude_history=exclude, mask=mask)
    np.testing.assert_array_equal(si, ti)
    np.testing.assert_array_equal(_bits(ss), _bits(ts))
    _same_ids(si, ref_ids)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_thin_equals_scan_at_the_row_block(monkeypatch, n):
    m, dim, k = 1025, 20, 33
    V, U, iptr, icol, _ = AR.grid_case(m, n, k, dim, 7950 + n)
    _, ref_ids, ref_sc = AR.audience64(V, U, iptr, icol, np.arange(n), k, True, None)
    with _ctx(V, U, iptr, icol) as ctx:
        monkeypatch.setenv(THIN, "0")
        si, ss = ctx.audience(k, items=np.arange(n))
        monkeypatch.setenv(THIN, "1000")
        assert _plan(dim, m, n, k)["thin"] == 1
        ti, ts = ctx.audience(k, items=np.arange(n))
    np.testing.assert_array_equal(si, ti)
    np.testing.assert_array_equal(_bits(ss), _bits(ts))
    _same_ids(si, ref_ids)
    np.testing.assert_array_equal(_bits(ss), _bits(_expect(ref_ids, ref_sc)))


@pytest.mark.parametrize("k", [100, 1024])
def test_split_pass_batch_independent(monkeypatch, k):
    m, dim = 5000, 64
    n = 2 * _plan(dim, m, 1, k)["queries_per_pass"] + 1
    rng = np.random.default_rng(7960 + k)
    U = (dim ** -0.25 * rng.standard_normal((m, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((n, dim))).astype(np.float32)
    iptr, icol = A.aux_eval(n, m, k, 7961)
    with _ctx(V, U, iptr, icol) as ctx:
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", "1")
        ctx.timing_reset()
        base_i, base_s = ctx.audience(k)
        assert ctx.timing("audience")[1] == 1       # one batch at the default budget
        flops, nbytes = ctx.work("audience")[:2]
        assert flops == 2.0 * n * m * dim
        assert nbytes == (_plan(dim, m, n, k, exclude=True)["passes"] * m + n) * dim * 4.0 + 8.0 * n * k
        _, ref_ids, _ = AR.audience64(V, U, iptr, icol, None, k, True, None)
        assert (base_i == ref_ids).mean() > 0.99    # the sweep itself is sane
        for path in ("1000", "0"):                  # the thin kernel, then the scan
            monkeypatch.setenv(THIN, path)
            for splits in ("1", "3", "7", None):
                if splits is None:
                    monkeypatch.delenv("FRECSYS_RECOMMEND_SPLITS")
                else:
                    monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", splits)
                ids, sc = ctx.audience(k)
                np.testing.assert_array_equal(ids, base_i)
                np.testing.assert_array_equal(_bits(sc), _bits(base_s))
            # 1 MiB of workspace: whatever the split count, 17 queries with
            # their lists, bits and outputs do not fit one batch
            monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
            pl = _plan(dim, m, n, k, exclude=True)
            assert pl["rows_per_batch"] < n and pl["workspace_bytes"] <= 1 << 20
            ctx.timing_reset()
            ids, sc = ctx.audience(k)
            assert ctx.timing("audience")[1] >= 2, "1 MiB must cut the queries into batches"
            np.testing.assert_array_equal(ids, base_i)
            np.testing.assert_array_equal(_bits(sc), _bits(base_s))
            monkeypatch.delenv("FRECSYS_RECOMMEND_WS_MB")


def _gauss_cases():
    """test_recommend_gpu._gauss_cases(): one case of aux_data.topk_cases() per
    table size, the dims rotated."""
    cases = A.topk_cases()
    out = []
    for i, m in enumerate(A.TOPK_M):
        same = [c for c in cases if c[0] == m]
        out.append(same[i % len(same)])
    return out


@pytest.mark.parametrize("m,rows,k,dim,seed", _gauss_cases())
def test_gaussian_float64(m, rows, k, dim, seed):
    # Ue: the item queries, V: the user table, (ep, ec): the ITEM-side CSR
    Ue, V, ep, ec, _, _, close = A.topk_inputs(m, rows, k, dim, seed)
    S, ref_ids, ref_sc = AR.audience64(Ue, V, ep, ec, None, k, True, None)
    with _ctx(Ue, V, ep, ec) as ctx:
        ids, scores = ctx.audience(k)
    assert close.sum() <= 0.05 * rows
    ok = ~close
    bad = np.nonzero(ok & (ids != ref_ids).any(axis=1))[0]
    assert len(bad) == 0, [(int(r), ids[r].tolist()[:40], ref_ids[r].tolist()[:40])
                           for r in bad[:2]]
    fin = np.isfinite(S)
    tol = 2e-6 * np.abs(S[fin]).max() if fin.any() else 0.0
    listed = ids >= 0
    rr = np.broadcast_to(np.arange(rows)[:, None], ids.shape)
    err = np.abs(scores[listed].astype(np.float64) - S[rr[listed], ids[listed]])
    print(f"audience gaussian m={m} rows={rows} k={k} dim={dim}: "
          f"max score err {err.max(initial=0):.3e} (bar {tol:.3e})")
    assert np.isfinite(S[rr[listed], ids[listed]]).all()
    assert (err <= tol).all()
    assert (scores[~listed] == -FLT_MAX).all()
    np.testing.assert_array_equal(listed.sum(axis=1), np.minimum(k, fin.sum(axis=1)))


def test_same_bits_as_score_pairs_and_recommend():
    nu, ni, dim = 40, 30, 20
    rng = np.random.default_rng(7970)
    U = rng.standard_normal((nu, dim)).astype(np.float32)
    V = rng.standard_normal((ni, dim)).astype(np.float32)
    with _ctx(V, U) as ctx:
        ai, asc = ctx.audience(nu, exclude_history=False)              # [ni, nu]
        ri, rs = ctx.recommend(fh.SIDE_USER, ni, exclude_history=False)  # [nu, ni]
        assert (np.sort(ai, axis=1) == np.arange(nu)).all()
        assert (np.sort(ri, axis=1) == np.arange(ni)).all()
        A_bits = np.zeros((ni, nu), np.uint32)
        np.put_along_axis(A_bits, ai.astype(np.int64), _bits(asc), axis=1)
        R_bits = np.zeros((nu, ni), np.uint32)
        np.put_along_axis(R_bits, ri.astype(np.int64), _bits(rs), axis=1)
        np.testing.assert_array_equal(A_bits, R_bits.T)
        uu, ii = np.meshgrid(np.arange(nu), np.arange(ni))
        pairs = ctx.score_pairs(fh.SIDE_USER, uu.reshape(-1), ii.reshape(-1)).reshape(ni, nu)
        np.testing.assert_array_equal(A_bits, _bits(pairs))


def test_item_row_subsets(monkeypatch):
    monkeypatch.setenv(THIN, "64")      # 400 items: the scan; 5: the thin kernel
    nu, ni, up, uc, ip, ic = make_quirk_data()
    idle, dim, k = 9, 32, 50
    assert ip[idle + 1] == ip[idle]
    rng = np.random.default_rng(7980)
    U = (dim ** -0.25 * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (dim ** -0.25 * rng.standard_normal((ni, dim))).astype(np.float32)
    with _ctx(V, U, ip, ic) as ctx:
        all_i, all_s = ctx.audience(k)
        assert all_i.shape == (ni, k)
        sub = rng.permutation(ni)[:90]
        sub = np.concatenate([sub, sub[:20], [idle, 399, idle]])   # item 399: half the users
        rng.shuffle(sub)
        it, sc = ctx.audience(k, items=sub)
        np.testing.assert_array_equal(it, all_i[sub])
        np.testing.assert_array_equal(_bits(sc), _bits(all_s[sub]))
        few = sub[:5]                                              # the thin kernel's lists
        assert _plan(dim, nu, len(few), k)["thin"] == 1 and _plan(dim, nu, ni, k)["thin"] == 0
        ti, ts = ctx.audience(k, items=few)
        np.testing.assert_array_equal(ti, all_i[few])
        np.testing.assert_array_equal(_bits(ts), _bits(all_s[few]))
        # no listed user is in the item's row; the idle item gets the plain ranking
        for r in (3, 11, 57, 399, 0):
            assert not set(all_i[r].tolist()) & set(ic[ip[r]:ip[r + 1]].tolist())
        pi, ps = ctx.audience(k, items=[idle], exclude_history=False)
        np.testing.assert_array_equal(pi[0], all_i[idle])
        np.testing.assert_array_equal(_bits(ps[0]), _bits(all_s[idle]))
    _, ref_ids, _ = AR.audience64(V, U, ip, ic, None, k, True, None)
    assert (all_i == ref_ids).all(axis=1).mean() > 0.97


def test_bad_arguments():
    nu, ni, dim = 50, 40, 16
    rng = np.random.default_rng(7990)
    U = rng.standard_normal((nu, dim)).astype(np.float32)
    V = rng.standard_normal((ni, dim)).astype(np.float32)
    with _ctx(V, U) as ctx:     # the ITEM CSR is never loaded

        def invalid(*a, **kw):
            with pytest.raises(fh.FrecsysError) as ei:
                ctx.audience(*a, **kw)
            assert ei.value.code == fh.ERR_INVALID, ei.value

        # ("a table without embeddings" and "no users" cannot be reached from
        # here: a context allocates both tables, of at least one row each)
        invalid(0, exclude_history=False)
        invalid(1025, exclude_history=False)
        invalid(5, items=[0, ni], exclude_history=False)    # in range for the users only
        invalid(5, items=[-1], exclude_history=False)
        invalid(5, items=[0], exclude_history=True)         # no ITEM CSR
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ids = np.zeros((ni + 1) * 5, np.int32)
        call = ctx.lib.frecsys_audience
        assert call(ctx.h, None, 1, 5, 2, None, P(ids), None) == fh.ERR_INVALID      # unknown flag
        assert call(ctx.h, None, 1, 5, -1, None, P(ids), None) == fh.ERR_INVALID
        assert call(ctx.h, None, ni + 1, 5, 0, None, P(ids), None) == fh.ERR_INVALID
        assert call(ctx.h, None, 1, 5, 0, None, None, None) == fh.ERR_INVALID        # null users
        assert call(ctx.h, None, -1, 5, 0, None, P(ids), None) == fh.ERR_INVALID
        assert call(None, None, 1, 5, 0, None, P(ids), None) == fh.ERR_INVALID
        # no queries: OK, and nothing is written (not even with null outputs)
        assert call(ctx.h, None, 0, 5, 0, None, None, None) == fh.OK
        # scores may be NULL; the context still answers
        assert call(ctx.h, None, ni, 5, 0, None, P(ids), None) == fh.OK
        it, sc = ctx.audience(5, exclude_history=False)
        np.testing.assert_array_equal(ids[:ni * 5].reshape(ni, 5), it)
        assert (it >= 0).all() and np.all(np.diff(sc, axis=1) <= 0)
        _, ref_ids, _ = AR.audience64(V, U, None, None, None, 5, False, None)
        assert (it == ref_ids).all(axis=1).mean() > 0.9
        np.testing.assert_array_equal(ctx.get_embeddings(fh.SIDE_USER), U)
        np.testing.assert_array_equal(ctx.get_embeddings(fh.SIDE_ITEM), V)


@pytest.mark.parametrize("thin", ["1000", "0"])
def test_buffers_are_owned_and_released(monkeypatch, thin):
    """The workspace is a buffer of the context: counted by
    "live_device_bytes", freed by release_workspaces (results unchanged
    afterwards) and with the context."""
    monkeypatch.setenv(THIN, thin)
    m, n, dim, k = 1025, 9, 64, 33
    rng = np.random.default_rng(7995)
    U = rng.standard_normal((m, dim)).astype(np.float32)
    V = rng.standard_normal((n, dim)).astype(np.float32)
    live = "live_device_bytes"
    pl = _plan(dim, m, n, k)
    with fh.Context(8, 1, 1) as witness:
        b0 = witness.counter(live)
        ctx = _ctx(V, U)
        made = witness.counter(live)
        ids, sc = ctx.audience(k, exclude_history=False)
        held = witness.counter(live)
        assert held - made >= pl["workspace_bytes"] >= n * (pl["splits"] * pl["slots"] * 8 + k * 8)
        ctx.release_workspaces()
        assert witness.counter(live) == made
        again_i, again_s = ctx.audience(k, exclude_history=False)
        assert witness.counter(live) == held
        np.testing.assert_array_equal(again_i, ids)
        np.testing.assert_array_equal(_bits(again_s), _bits(sc))
        ctx.close()
        assert witness.counter(live) == b0
