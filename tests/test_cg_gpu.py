"""The conjugate-gradient solve path (frecsys_solve_side_cg, csrc/cg.hip)
against the float64 numpy CG of tests/cg_ref.py.

Shapes: dims 8 .. 256 (padded and unpadded), about 600 rows on the other
side, solved sides of 1 / 33 / 70 rows (no multiple of the kernel's batch of
16), two empty histories, history lengths 1, 3, 64, 129, 300 and the
kernel's row chunk +- 1 (cg_ref.row_chunk).  Bar: rel_rows < TOL_ROW = 1e-4;
the float32 rounding of the recurrence itself stays below TOL_ROW / 4 on
these fixtures (tests/test_cg_cpu.py).
"""
import numpy as np
import pytest

import cg_ref as C
import frecsys_hip as fh
from conftest import rel_rows

pytestmark = pytest.mark.gpu

TOL_ROW = C.TOL_ROW
CASES = C.gpu_cases()
IDS = [c[0] for c in CASES]
ARGS = [c[1] for c in CASES]


def _context(case, side=None, n_rows=None, ptr=None, col=None, E0=None):
    """A context holding `case`'s other side and Gramian and the given rows
    (default: the case's own) loaded as `side`."""
    side = case.side if side is None else side
    ptr = case.ptr if ptr is None else ptr
    col = case.col if col is None else col
    E0 = case.E0 if E0 is None else E0
    n = len(ptr) - 1
    if side == fh.SIDE_ITEM:
        ctx = fh.Context(case.dim, C.N_OTHER, n, device=0, parity_quirks=case.quirk)
        other = fh.SIDE_USER
    else:
        ctx = fh.Context(case.dim, n, C.N_OTHER, device=0, parity_quirks=case.quirk)
        other = fh.SIDE_ITEM
    ctx.load_csr(side, ptr, col)
    ctx.set_embeddings(other, case.X)
    ctx.set_embeddings(side, E0)
    ctx.gramian(other, case.gram_weights, fetch=False)
    return ctx


def _solve(ctx, case, side=None, max_iterations=100, tolerance=1e-10, rows=slice(None)):
    side = case.side if side is None else side
    kw = dict(reg_exp=case.reg_exp, alpha=case.alpha)
    if case.kind == C.KIND_U:
        kw["entity_weight"] = case.omega[rows]
    if case.kind == C.KIND_V:
        kw["entity_reg"] = case.item_reg[rows]
        kw["other_weight"] = case.nu
    ctx.solve_side_cg(side, case.kind, case.reg, case.w, max_iterations, tolerance, **kw)
    return ctx.get_embeddings(side), ctx.cg_iterations(side)


def _check_rows(case, x, ref, what):
    err = rel_rows(x, ref)
    print(f"{what}: max row rel err {err.max():.2e}")
    assert err.max() < TOL_ROW, (what, float(err.max()), int(err.argmax()))
    for e in case.empty:  # untouched, bit for bit
        np.testing.assert_array_equal(x[e], case.E0[e])


@pytest.mark.parametrize("args", ARGS, ids=IDS)
def test_truncated_iterates(args):
    """tolerance 0, max_iterations 1 / 2 / 5: the iterate of the float64 CG
    (5 - 80 % away from the exact solve: pins Jacobi, the zero start and the
    coefficients; not reachable through the LLT path)."""
    case = C.get_case(args)
    ctx = _context(case)
    solved = np.ones(case.n_rows, bool)
    solved[case.empty] = False
    for cap in C.CAPS:
        ctx.set_embeddings(case.side, case.E0)
        x, it = _solve(ctx, case, max_iterations=cap, tolerance=0.0)
        _check_rows(case, x, case.trunc[cap], f"cap {cap}")
        assert (it[solved] == cap).all(), it
        assert (it[~solved] == -1).all(), it
    away = rel_rows(case.trunc[1], case.direct)[solved]
    assert away.max() > 0.05  # the test cannot pass through a direct solve
    ctx.close()


@pytest.mark.parametrize("args", ARGS, ids=IDS)
def test_converged_matches_direct(args):
    """Defaults (1e-10, 100): the float64 direct solve."""
    case = C.get_case(args)
    ctx = _context(case)
    before = ctx.counter("cg_unconverged")
    x, it = _solve(ctx, case)
    _check_rows(case, x, case.direct, "converged")
    assert it.max() < 100
    assert ctx.counter("cg_unconverged") == before
    ctx.close()


@pytest.mark.parametrize("args", [a for a in ARGS if a[3] > 1],
                         ids=[i for i, a in zip(IDS, ARGS) if a[3] > 1])
def test_stopping_rule(args):
    """tolerance 1e-3: true float64 relative residual <= 2e-3 on every row
    (the recurrence residual drifts from it by O(eps cond i) << 1e-3), nobody
    stops at the cap, the per-row iteration counts differ."""
    case = C.get_case(args)
    ctx = _context(case)
    un0, it0 = ctx.counter("cg_unconverged"), ctx.counter("cg_iterations")
    ctx.timing_reset()
    x, it = _solve(ctx, case, max_iterations=100, tolerance=1e-3)
    res = C.residual_side(case, x)
    print(f"max true residual {res.max():.2e}, iterations {it[it >= 0].min()}..{it.max()}")
    assert res.max() <= 2e-3
    assert ctx.counter("cg_unconverged") == un0
    solved = it >= 0
    assert (it[solved] < 100).all()
    assert len(set(it[solved].tolist())) > 1
    assert ctx.counter("cg_iterations") - it0 == int(it[solved].sum())
    # frecsys_work("<solve>.cg"): sum_e i_e (2 d^2 + 4 h_e d), i_e (h_e d 4 + h_e 4)
    h = np.diff(case.ptr)[solved].astype(np.float64)
    i = it[solved].astype(np.float64)
    d = float(case.dim)
    key = ("solve_user" if case.side == fh.SIDE_USER else "solve_item") + ".cg"
    fl, by, ne, nl = ctx.work(key)
    assert fl == pytest.approx(float((i * (2 * d * d + 4 * h * d)).sum()), rel=1e-12)
    assert by == pytest.approx(float((i * (h * d * 4 + h * 4)).sum()), rel=1e-12)
    assert ne == int(solved.sum()) and nl == 1
    assert ctx.timing(key)[1] == 1
    ctx.close()


@pytest.mark.parametrize("dim", C.DIMS)
def test_zero_rhs(dim):
    """WEIGHTED_U with omega = 0: b = 0, so an exactly zero row, 0 iterations."""
    case = C.Case(C.KIND_U, C.SIDE_USER, dim, 33)
    case.omega = case.omega.copy()
    zero = [0, 4, 20]
    case.omega[zero] = 0.0
    ctx = _context(case)
    x, it = _solve(ctx, case)
    for e in zero:
        assert not x[e].any() and it[e] == 0
    ref, _, _ = C.cg_side(case, 100, 1e-10)
    _check_rows(case, x, ref, "zero rhs")
    ctx.close()


def test_max_iterations_zero():
    """max_iterations = 0: x = 0 (Eigen), counted as stopped at the cap."""
    case = C.get_case((C.KIND_IALS, C.SIDE_USER, 64, 33, False))
    ctx = _context(case)
    un0 = ctx.counter("cg_unconverged")
    x, it = _solve(ctx, case, max_iterations=0)
    solved = np.diff(case.ptr) > 0
    assert not x[solved].any() and (it[solved] == 0).all() and (it[~solved] == -1).all()
    np.testing.assert_array_equal(x[~solved], case.E0[~solved])
    assert ctx.counter("cg_unconverged") - un0 == int(solved.sum())
    ctx.close()


def _subset(case, rows):
    hs = np.diff(case.ptr)[rows]
    ptr = np.concatenate([[0], np.cumsum(hs)]).astype(np.int64)
    col = np.concatenate([case.col[case.ptr[r]:case.ptr[r + 1]] for r in rows]
                         + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, col


@pytest.mark.parametrize("kind,side,quirk", [(C.KIND_IALS, C.SIDE_USER, False),
                                             (C.KIND_U, C.SIDE_USER, False),
                                             (C.KIND_V, C.SIDE_ITEM, True)])
@pytest.mark.parametrize("dim", C.DIMS)
def test_bits_independent_of_batch(dim, kind, side, quirk):
    """The same rows on a side of 70 and on a side holding a subset of them
    (other batches, other slots, another grid): identical bits."""
    case = C.get_case((kind, side, dim, 70, quirk))
    ctx = _context(case)
    full, it_full = _solve(ctx, case, max_iterations=7, tolerance=1e-4)
    ctx.close()
    rows = np.array([r for r in range(70) if r % 3 != 1][5:])
    ptr, col = _subset(case, rows)
    ctx = _context(case, ptr=ptr, col=col, E0=case.E0[rows])
    sub, it_sub = _solve(ctx, case, max_iterations=7, tolerance=1e-4, rows=rows)
    ctx.close()
    np.testing.assert_array_equal(sub, full[rows])
    np.testing.assert_array_equal(it_sub, it_full[rows])


@pytest.mark.parametrize("dim", [8, 100, 256])
def test_bits_independent_of_world(dim):
    """World 2 (two contexts of one device, external exchange: each solves
    its own shard) against world 1: identical bits; a rank's cg_iterations
    hold -1 for the other rank's rows."""
    case = C.get_case((C.KIND_IALS, C.SIDE_USER, dim, 70, False))
    ctx = _context(case)
    one, it_one = _solve(ctx, case, max_iterations=7, tolerance=1e-4)
    ctx.close()
    full = case.E0.copy()
    its = np.full(case.n_rows, -1, np.int32)
    covered = 0
    for r in range(2):
        c = fh.Context(case.dim, case.n_rows, C.N_OTHER, device=0)
        c.comm_init(2, r, None)
        c.load_csr(fh.SIDE_USER, case.ptr, case.col)
        c.set_embeddings(fh.SIDE_ITEM, case.X)
        c.set_embeddings(fh.SIDE_USER, case.E0)
        c.set_gramian(fh.SIDE_ITEM, _gram_of(case))
        x, it = _solve(c, case, max_iterations=7, tolerance=1e-4)
        lo, hi = c.shard_range(fh.SIDE_USER)
        assert (it[:lo] == -1).all() and (it[hi:] == -1).all()
        np.testing.assert_array_equal(x[:lo], case.E0[:lo])  # only its own rows written
        np.testing.assert_array_equal(x[hi:], case.E0[hi:])
        full[lo:hi], its[lo:hi] = x[lo:hi], it[lo:hi]
        covered += hi - lo
        c.close()
    assert covered == case.n_rows
    np.testing.assert_array_equal(full, one)
    np.testing.assert_array_equal(its, it_one)


def _gram_of(case):
    """The Gramian the single context formed, for the ranks' set_gramian."""
    c = fh.Context(case.dim, 1, C.N_OTHER, device=0)
    c.set_embeddings(fh.SIDE_ITEM, case.X)
    G = c.gramian(fh.SIDE_ITEM, case.gram_weights)
    c.close()
    return G


@pytest.mark.parametrize("dim", [20, 256])
def test_eval_side_matches_user_side(dim):
    """The fold-in through frecsys_solve_side_cg(EVAL) = the USER-side solve
    of the same histories, bit for bit; EVAL's empty rows stay zero."""
    case = C.get_case((C.KIND_IALS, C.SIDE_USER, dim, 33, False))
    ctx = _context(case)
    xu, iu = _solve(ctx, case, max_iterations=5, tolerance=1e-4)
    ctx.load_csr(fh.SIDE_EVAL, case.ptr, case.col)
    xe, ie = _solve(ctx, case, side=fh.SIDE_EVAL, max_iterations=5, tolerance=1e-4)
    solved = np.diff(case.ptr) > 0
    np.testing.assert_array_equal(xe[solved], xu[solved])
    np.testing.assert_array_equal(ie, iu)
    assert not xe[~solved].any()
    assert ctx.timing("solve_eval.cg")[1] == 1
    ctx.close()


@pytest.mark.parametrize("kind", [C.KIND_IALS, C.KIND_U, C.KIND_V])
def test_one_row_context_with_given_gramian(kind):
    """The calls the static Project / ProjectU / ProjectV make with use_cg
    (model_base.h ProjectOnDevice): a one-row context, the caller's Gramian
    (frecsys_set_gramian), `reg` as the final lambda (lambda_is_reg)."""
    case = C.Case(kind, C.SIDE_USER, 100, 1)
    case.lam = lambda e, h: C.R._f32(0.25)
    ctx = fh.Context(case.dim, 1, C.N_OTHER, device=0, parity_quirks=True)
    ctx.load_csr(fh.SIDE_USER, case.ptr, case.col)
    ctx.set_embeddings(fh.SIDE_ITEM, case.X)
    ctx.set_gramian(fh.SIDE_ITEM, C.gram(case, np.float64).astype(np.float32))
    kw = {}
    if kind == C.KIND_U:
        kw["entity_weight"] = case.omega
    if kind == C.KIND_V:
        case.quirk = True
        kw.update(entity_reg=np.zeros(1, np.float32), other_weight=case.nu)
    for cap, tol in ((2, 0.0), (100, 1e-10)):
        ctx.solve_side_cg(fh.SIDE_USER, kind, 0.25, case.w, cap, tol, lambda_is_reg=True, **kw)
        ref, it_ref, _ = C.cg_side(case, cap, tol)
        err = rel_rows(ctx.get_embeddings(fh.SIDE_USER), ref)
        print(f"kind {kind} cap {cap}: {err.max():.2e}")
        assert err.max() < TOL_ROW
        if tol == 0.0:
            assert ctx.cg_iterations(fh.SIDE_USER)[0] == cap
    ctx.close()


def test_limits_and_invalid_parameters():
    case = C.get_case((C.KIND_IALS, C.SIDE_USER, 8, 33, False))
    ctx = _context(case)
    for kw in (dict(max_iterations=-1), dict(tolerance=-1e-3), dict(tolerance=float("nan"))):
        with pytest.raises(fh.FrecsysError) as e:
            ctx.solve_side_cg(fh.SIDE_USER, fh.KIND_IALS, case.reg, case.w, **kw)
        assert e.value.code == fh.ERR_INVALID
    for kind in (fh.KIND_CVAR_GRAD_U, fh.KIND_CVAR_GRAD_V):
        with pytest.raises(fh.FrecsysError) as e:
            ctx.solve_side_cg(fh.SIDE_USER, kind, case.reg, case.w)
        assert e.value.code == fh.ERR_INVALID
    np.testing.assert_array_equal(ctx.get_embeddings(fh.SIDE_USER), case.E0)  # nothing ran
    assert (ctx.cg_iterations(fh.SIDE_USER) == -1).all()
    ctx.close()
    wide = fh.Context(300, 4, 16, device=0)
    wide.load_csr(fh.SIDE_USER, np.array([0, 1, 2, 3, 4]), np.array([0, 1, 2, 3]))
    wide.init_embeddings(1, 0.1)
    wide.gramian(fh.SIDE_ITEM, fetch=False)
    with pytest.raises(fh.FrecsysError) as e:
        wide.solve_side_cg(fh.SIDE_USER, fh.KIND_IALS, 0.003, 0.1)
    assert e.value.code == fh.ERR_UNSUPPORTED and "256" in str(e.value)
    wide.close()
