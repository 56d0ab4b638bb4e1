"""frecsys_explain (csrc/explain.hip, csrc/serve.hip) against the float64
reference of tests/explain_ref.py.

Fixtures (explain_ref.ROWS): about 600 items, dims 8 .. 256 (Dp 8, 32, 64, 128,
224, 256), kinds IALS and WEIGHTED_U (log-uniform omega), history lengths 0, 1,
31, 32, 33, chunk - 1, chunk, chunk + 1, 300, 2 chunk + 5 (chunk: the rows one
sweep of the kernel's second pass takes), 0 .. 70 targets per row, some inside
the history, some repeated.

Bars.  Per pair ||contrib - ref|| / ||ref|| < TOL_ROW = 1e-4 over the history;
per score |s - s_ref| <= TOL_ROW ||v_t|| ||x_ref|| (the bound the per-row solve
bar implies for a dot product).  The float32 rounding of the kernel's steps
stays below TOL_ROW / 4 on these fixtures (tests/test_explain_cpu.py).  The
worst margins go to parity_report.jsonl (test = "explain").
"""
import ctypes

import numpy as np
import pytest

import cg_ref as C
import explain_ref as X
import frecsys_hip as fh
from test_models_gpu import report

pytestmark = pytest.mark.gpu

TOL_ROW = X.TOL_ROW
U, E, I = fh.SIDE_USER, fh.SIDE_EVAL, fh.SIDE_ITEM
CASES = [(k, d) for d in X.DIMS for k in X.KINDS]
IDS = [f"{'ials' if k == C.KIND_IALS else 'u'}-d{d}" for k, d in CASES]


def _context(case, side):
    if side == U:
        ctx = fh.Context(case.dim, case.n_rows, X.N_OTHER, device=0)
    else:
        ctx = fh.Context(case.dim, 1, X.N_OTHER, device=0)
    ctx.load_csr(side, case.ptr, case.col)
    ctx.set_embeddings(I, case.X)
    ctx.gramian(I, None, fetch=False)
    return ctx


def _explain(ctx, case, side, tgt_ptr=None, tgt=None, rows=None, top=5, full=True):
    tgt_ptr = case.tgt_ptr if tgt_ptr is None else tgt_ptr
    tgt = case.tgt if tgt is None else tgt
    return ctx.explain(side, case.kind, case.reg, case.w, tgt_ptr, tgt, rows=rows, top=top,
                       full=full, **case.solve_kw())


_results = {}


def _result(kind, dim, side):
    """(score, top_items, top_contrib, full, full_ptr) of the case's own call
    with top = 5, once per process."""
    key = (kind, dim, side)
    if key not in _results:
        case = X.get_case(kind, dim)
        with _context(case, side) as ctx:
            _results[key] = _explain(ctx, case, side)
    return _results[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(_bits(x), _bits(y))


def _pairs(case):
    """(row, target index) of every pair in order."""
    return [(e, t) for e in range(case.n_rows) for t in range(X.ROWS[e][1])]


@pytest.mark.parametrize("side", [U, E], ids=["user", "eval"])
@pytest.mark.parametrize("kind,dim", CASES, ids=IDS)
def test_against_float64(kind, dim, side):
    case = X.get_case(kind, dim)
    score, _, _, full, fp = _result(kind, dim, side)
    assert len(score) == case.tgt_ptr[-1] and len(fp) == len(score) + 1
    worst_c = worst_s = 0.0
    for p, (e, t) in enumerate(_pairs(case)):
        contrib, sref, x = case.ref[e]
        got = full[fp[p]:fp[p + 1]]
        assert len(got) == X.ROWS[e][0]
        if len(got) == 0:
            assert score[p] == 0.0
            continue
        err = np.linalg.norm(got.astype(np.float64) - contrib[:, t]) / np.linalg.norm(contrib[:, t])
        bound = np.linalg.norm(case.X[case.targets(e)[t]].astype(np.float64)) * np.linalg.norm(x)
        serr = abs(float(score[p]) - sref[t]) / bound
        worst_c, worst_s = max(worst_c, err), max(worst_s, serr)
    print(f"worst pair rel err {worst_c:.2e}, worst score err / (|v| |x|) {worst_s:.2e}")
    report(test="explain", kind=int(kind), dim=int(dim), side=int(side), tol=TOL_ROW,
           worst_contrib_rel=worst_c, worst_score_scaled=worst_s)
    assert worst_c < TOL_ROW
    assert worst_s <= TOL_ROW


@pytest.mark.parametrize("kind,dim", CASES, ids=IDS)
def test_against_solve_and_score_pairs(kind, dim):
    """solve_side(EVAL) then score_pairs: the same scores within twice the
    bound (both sides carry rounding)."""
    case = X.get_case(kind, dim)
    score = _result(kind, dim, E)[0]
    with _context(case, E) as ctx:
        ctx.solve_side(E, case.kind, case.reg, case.w, **case.solve_kw())
        rows = np.repeat(np.arange(case.n_rows), np.diff(case.tgt_ptr))
        lib_score = ctx.score_pairs(E, rows, case.tgt)
    worst = 0.0
    for p, (e, t) in enumerate(_pairs(case)):
        if X.ROWS[e][0] == 0:
            assert score[p] == 0.0 and lib_score[p] == 0.0  # EVAL rows start at zero
            continue
        bound = (np.linalg.norm(case.X[case.targets(e)[t]].astype(np.float64)) *
                 np.linalg.norm(case.ref[e][2]))
        worst = max(worst, abs(float(score[p]) - float(lib_score[p])) / bound)
    print(f"worst |explain - score_pairs| / (|v| |x|) {worst:.2e}")
    assert worst <= 2 * TOL_ROW


@pytest.mark.parametrize("kind,dim", CASES, ids=IDS)
def test_lists_are_exact(kind, dim):
    """top_items / top_contrib are top_of of the same call's full, bit for bit,
    with the -1 / 0 fill behind short and empty histories."""
    case = X.get_case(kind, dim)
    with _context(case, U) as ctx:
        for top in X.TOPS:
            score, items, vals, full, fp = _explain(ctx, case, U, top=top)
            assert items.shape == vals.shape == (len(score), top)
            for p, (e, t) in enumerate(_pairs(case)):
                pos, ref_vals = X.top_of(full[fp[p]:fp[p + 1]], top)
                ref_items = np.where(pos >= 0, case.hist(e)[np.maximum(pos, 0)] if len(case.hist(e))
                                     else -1, -1).astype(np.int32)
                np.testing.assert_array_equal(items[p], ref_items)
                np.testing.assert_array_equal(_bits(vals[p]), _bits(ref_vals.astype(np.float32)))
                h = X.ROWS[e][0]
                assert (items[p, h:] == -1).all() and not vals[p, h:].any()
            _same((score, full), (_result(kind, dim, U)[0], _result(kind, dim, U)[3]))  # `top` changes nothing


@pytest.mark.parametrize("kind,dim", CASES, ids=IDS)
def test_independence(kind, dim, monkeypatch):
    case = X.get_case(kind, dim)
    base = _result(kind, dim, U)
    _same(base, _result(kind, dim, E))  # USER versus EVAL with the same CSR
    score, items, vals, full, fp = base
    n = case.n_rows
    pair0 = case.tgt_ptr
    with _context(case, U) as ctx:
        # rows permuted
        perm = np.random.default_rng(5).permutation(n)
        tp = np.concatenate([[0], np.cumsum(np.diff(pair0)[perm])]).astype(np.int64)
        tg = np.concatenate([case.targets(e) for e in perm]).astype(np.int32)
        got = _explain(ctx, case, U, tp, tg, rows=perm)
        for i, e in enumerate(perm):
            a, b = slice(tp[i], tp[i + 1]), slice(pair0[e], pair0[e + 1])
            _same((got[0][a], got[1][a], got[2][a]), (score[b], items[b], vals[b]))
            _same((got[3][got[4][tp[i]]:got[4][tp[i + 1]]],), (full[fp[pair0[e]]:fp[pair0[e + 1]]],))
        # the call split into two
        cut = 8
        lo = _explain(ctx, case, U, pair0[:cut + 1], case.tgt[:pair0[cut]], rows=np.arange(cut))
        hi = _explain(ctx, case, U, pair0[cut:] - pair0[cut], case.tgt[pair0[cut]:],
                      rows=np.arange(cut, n))
        _same(tuple(np.concatenate([x, y]) for x, y in zip(lo[:4], hi[:4])), base[:4])
        # 70 targets as 70 single-target repeats of the row
        e = [m for _, m in X.ROWS].index(70)
        m = X.ROWS[e][1]
        got = _explain(ctx, case, U, np.arange(m + 1), case.targets(e), rows=np.full(m, e))
        b = slice(pair0[e], pair0[e + 1])
        _same(got[:3], (score[b], items[b], vals[b]))
        _same((got[3],), (full[fp[pair0[e]]:fp[pair0[e + 1]]],))
        # a workspace budget that cuts the call into several batches
        rep = 8
        rows = np.tile(np.arange(n), rep)
        tp = np.concatenate([[0], np.cumsum(np.tile(np.diff(pair0), rep))]).astype(np.int64)
        tg = np.tile(case.tgt, rep)
        assert 4 * int(np.repeat(np.diff(case.ptr)[rows], np.diff(tp)).sum()) > 1 << 20
        wide = _explain(ctx, case, U, tp, tg, rows=rows)
        before = ctx.timing("explain")[1]
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", "1")
        tight = _explain(ctx, case, U, tp, tg, rows=rows)
        monkeypatch.delenv("FRECSYS_RECOMMEND_WS_MB")
        assert ctx.timing("explain")[1] - before > 1  # more than one batch
        _same(tight, wide)
        _same(tuple(x[:len(y)] for x, y in zip(wide[:4], base[:4])), base[:4])


def _raw(ctx, **kw):
    """frecsys_explain through the C-ABI with one defect; (code, message)."""
    a = dict(side=U, kind=fh.KIND_IALS, rows=None, n=2, tgt_ptr=np.array([0, 1, 3], np.int64),
             tgt=np.array([2, 0, 4], np.int32), top=3)
    a.update(kw)
    p = fh._SolveParams(a["kind"], 0.003, 1.0, 0.1, 0.0, 0.0, 0, 0, None, None, None)
    score = np.zeros(8, np.float32)
    items = np.zeros(8 * 32, np.int32)
    vals = np.zeros(8 * 32, np.float32)
    P = fh._ptr
    rc = ctx.lib.frecsys_explain(ctx.h, a["side"], ctypes.byref(p), P(a["rows"]), a["n"],
                                 P(a["tgt_ptr"]), P(a["tgt"]), a["top"], P(score), P(items),
                                 P(vals), None)
    return rc, ctx.lib.frecsys_last_error(ctx.h).decode()


DEFECTS = [
    (dict(side=I), fh.ERR_INVALID, "explain: side must be USER or EVAL"),
    (dict(kind=fh.KIND_WEIGHTED_V), fh.ERR_INVALID, "explain: kind must be IALS or WEIGHTED_U"),
    (dict(kind=fh.KIND_CVAR_GRAD_U), fh.ERR_INVALID, "explain: kind must be IALS or WEIGHTED_U"),
    (dict(top=0), fh.ERR_INVALID, "explain: top must be in [1, 32]"),
    (dict(top=33), fh.ERR_INVALID, "explain: top must be in [1, 32]"),
    (dict(tgt_ptr=np.array([0, 3, 2], np.int64)), fh.ERR_INVALID, "explain: cand_ptr not monotone"),
    (dict(tgt=np.array([2, 0, 5], np.int32)), fh.ERR_INVALID, "explain: candidate id 5 out of range"),
    (dict(tgt=np.array([2, -1, 4], np.int32)), fh.ERR_INVALID, "explain: candidate id -1 out of"),
    (dict(rows=np.array([0, 6], np.int64)), fh.ERR_INVALID, "explain: row id 6 out of range"),
    (dict(n=7, tgt_ptr=np.arange(8, dtype=np.int64), tgt=np.zeros(7, np.int32)), fh.ERR_INVALID,
     "explain: more rows than the side has"),
    (dict(n=-1), fh.ERR_INVALID, "explain: negative row count"),
    (dict(side=E), fh.ERR_INVALID, "explain: no CSR loaded on the side"),
]


def test_argument_checks():
    rng = np.random.default_rng(3)
    with fh.Context(8, 6, 5, device=0) as ctx:
        ctx.load_csr(U, np.array([0, 2, 3, 3, 4, 6, 7]), np.array([0, 1, 2, 3, 4, 0, 1]))
        ctx.set_embeddings(I, rng.standard_normal((5, 8)).astype(np.float32))
        ctx.gramian(I, None, fetch=False)
        assert _raw(ctx)[0] == fh.OK  # the arguments every defect starts from
        before = ctx.timing("explain")
        assert before[1] >= 1
        for kw, code, msg in DEFECTS:
            rc, text = _raw(ctx, **kw)
            assert rc == code and text.startswith(msg), (kw, rc, text)
        assert ctx.timing("explain") == before  # a rejected call launches nothing
        # zero rows / zero targets: OK without a launch
        assert _raw(ctx, n=0)[0] == 0
        assert _raw(ctx, tgt_ptr=np.zeros(3, np.int64))[0] == 0
        assert ctx.timing("explain") == before
    with fh.Context(288, 2, 5, device=0) as ctx:  # beyond the dims built
        ctx.load_csr(U, np.array([0, 1, 2]), np.array([0, 1]))
        rc, text = _raw(ctx)
        assert rc == fh.ERR_UNSUPPORTED and text.startswith("explain: explanations are built for dim <= 256")
        assert ctx.timing("explain") == (0.0, 0)


def test_work_is_booked():
    kind, dim = C.KIND_IALS, 64
    case = X.get_case(kind, dim)
    with _context(case, U) as ctx:
        _explain(ctx, case, U, full=False)
        fl, by, ent, _ = ctx.work("explain")
    d = float(dim)
    want = sum(h * d * d + d ** 3 / 3 + 2 * d * d * m + 2 * h * d * m
               for h, m in X.ROWS if h and m)
    assert ent == case.n_rows and by > 0
    np.testing.assert_allclose(fl, want, rtol=1e-12)
