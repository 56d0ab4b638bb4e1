"""The kernels around the solve at their seams, against float64: the Gramian
(csrc/gramian.hip, wide.hip), the per-user loss (loss.hip, wide.hip), the
train statistics and the snapshot residual.  Inputs: tests/aux_data.py; the
references: tests/numpy_ref.py; the conditions under which the bars mean
anything: tests/test_aux_cpu.py.  The top-K cases are in test_topk_gpu.py.

Gramian   row counts 1 (one row), 31 | 32 | 33 (the 32-row chunk of a leaf),
          63 | 64 | 65 (one 64-row leaf | two), 97 (a chunk edge + 1), 1024 |
          1025 (16 leaves, one per group | 17: groups of 1 and 2 leaves), 1089
          (18 leaves, the last of one row), 32769 (96-row leaves, 342 of
          them); at Dp = 512 / 1024: 1, 15 | 16 | 17, 255 | 256 | 257 (one
          leaf | two), 4097.  Unweighted and weighted (every 7th weight 0).
          Bar: |G - G64|_ij <= 2e-6 sqrt(G64_ii G64_jj) for every element
          (aux_data.gram_bar: 4 x the fp32 oracle's own error where that is
          past a quarter of 2e-6), and G exactly symmetric.
loss      aux_users with scaled embeddings: every row within 2e-5 of float64,
          idle rows exactly 0; SIDE_EVAL on 70 rows; the rows of an earlier
          EVAL call or an earlier CSR must not show through.
stats     observed / unobserved / norms within 1e-5; the residual within 1e-5
          and exactly 0 on an unchanged snapshot.
One line per case goes to parity_report.jsonl (test = "aux").
"""
import itertools
import types

import numpy as np
import pytest

import aux_data as A
import numpy_ref as R
from test_models_gpu import report

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

LOSS_TOL = 2e-5
STATS_TOL = 1e-5
LOSS_DIMS = [8, 16, 20, 64, 96, 128, 160, 224, 256, 500, 1000]
# padded dim: where u^T G u comes from -- the loss kernel itself (Dp <= 16),
# quad_kernel (32), or that many column-block partials of the rotation kernel
# (1..4 at Dp <= 256, one per 128 columns at Dp = 512 / 1024)
QUAD_PATH = {8: "kernel", 16: "kernel", 32: "quad", 64: 1, 96: 2, 128: 1, 160: 3, 224: 4, 256: 2,
             512: 4, 1024: 8}
# (rows per leaf, leaves) the row counts were chosen for (Dp <= 256)
GRAM_PLAN = {64: (64, 1), 65: (64, 2), 1024: (64, 16), 1025: (64, 17), 1089: (64, 18),
             32769: (96, 342)}


# ---------------------------------------------------------------- Gramian
@pytest.mark.parametrize("dim,n", A.gram_cases())
def test_gramian_seams_vs_float64(dim, n):
    X, w = A.gram_rows(dim, n)
    rpl, nleaf, ngroup, _, _ = fh.gram_plan(dim, n)
    if fh.padded_dim(dim) <= 256 and n in GRAM_PLAN:
        assert (rpl, nleaf) == GRAM_PLAN[n]
    if n == 1089:
        assert n - (nleaf - 1) * rpl == 1  # the last leaf holds one row
    if n == 1025:
        assert ngroup == 16  # 17 leaves in 16 groups: one group sums two leaves
    bar = A.gram_bar(dim, n)
    with fh.Context(dim, n, 1) as ctx:  # no CSR: the Gramian needs none
        ctx.set_embeddings(fh.SIDE_USER, X)
        got = [(wt, ctx.gramian(fh.SIDE_USER, weights=wt)) for wt in (None, w)]
    errs = []
    for wt, G in got:
        e = A.gram_err(G, R.gram64(X, wt))
        errs.append(e)
        print(f"aux gramian d={dim} n={n} {'plain' if wt is None else 'weighted'}: {e:.2e} "
              f"(bar {bar:.2e}; leaves {nleaf} x {rpl}, groups {ngroup})")
        report(test="aux", entry="gramian", dim=dim, rows=n, weighted=wt is not None, err=e,
               bar=bar, margin=bar / max(e, 1e-30), rpl=rpl, leaves=nleaf, groups=ngroup)
    for (wt, G), e in zip(got, errs):
        np.testing.assert_array_equal(G, G.T)
        assert e <= bar, (e, bar, "plain" if wt is None else "weighted")


@pytest.mark.parametrize("dim", [16, 64, 256, 500, 1000])
@pytest.mark.parametrize("n", [65, 257])
def test_gramian_snapshot_then_plain(dim, n):
    """from_snapshot and the reuse cache: a snapshot Gramian must not be taken
    for the embeddings' own, and an unchanged table gives the same bits."""
    X, _ = A.gram_rows(dim, n)
    Y = A.gram_rows(dim + 1, n)[0][:, :dim].copy()
    bar = A.gram_bar(dim, n)
    with fh.Context(dim, n, 1) as ctx:
        ctx.set_embeddings(fh.SIDE_USER, X)
        G0 = ctx.gramian(fh.SIDE_USER)
        ctx.snapshot(fh.SIDE_USER)
        ctx.set_embeddings(fh.SIDE_USER, Y)
        Gs = ctx.gramian(fh.SIDE_USER, from_snapshot=True)
        G1 = ctx.gramian(fh.SIDE_USER)
        G2 = ctx.gramian(fh.SIDE_USER)
        held = ctx.get_gramian(fh.SIDE_USER)
    ex, ey = A.gram_err(G0, R.gram64(X)), A.gram_err(G1, R.gram64(Y))
    es = A.gram_err(Gs, R.gram64(X))
    report(test="aux", entry="gramian_sequence", dim=dim, rows=n, err=max(ex, es, ey), bar=bar,
           margin=bar / max(ex, es, ey, 1e-30))
    assert ex <= bar and es <= bar and ey <= bar, (ex, es, ey)
    np.testing.assert_array_equal(Gs, G0)  # the same rows, the same sum
    np.testing.assert_array_equal(G2, G1)
    np.testing.assert_array_equal(held, G1)
    assert A.gram_err(G1, R.gram64(X)) > 0.01  # and X, Y are different tables


# ---------------------------------------------------------------- user loss
_loss = {}


def _loss_case(dim):
    if dim not in _loss:
        nu, ni, up, uc, ip, ic = A.aux_users()
        U, V = A.scaled_embeddings(dim, nu, ni, dim)
        ep, ec = A.eval_slice(up, uc)
        _loss[dim] = types.SimpleNamespace(nu=nu, ni=ni, up=up, uc=uc, ip=ip, ic=ic, U=U, V=V,
                                           G64=R.gram64(V), ep=ep, ec=ec, Ue=U[1:1 + A.EVAL_ROWS],
                                           live=np.diff(up) > 0, ref={})
    return _loss[dim]


def _loss_ref(c, side, beta, half):
    k = (side, beta, half)
    if k not in c.ref:
        if side == fh.SIDE_USER:
            r = R.user_loss_side(c.up, c.uc, c.U, c.V, c.G64, beta, half)
        else:
            r = R.user_loss_side(c.ep, c.ec, c.Ue, c.V, c.G64, beta, half)
        r.setflags(write=False)
        c.ref[k] = r
    return c.ref[k]


def _loss_ctx(c, dim):
    ctx = fh.Context(dim, c.nu, c.ni)
    ctx.load_csr(fh.SIDE_USER, c.up, c.uc)
    ctx.load_csr(fh.SIDE_ITEM, c.ip, c.ic)
    ctx.set_embeddings(fh.SIDE_USER, c.U)
    ctx.set_embeddings(fh.SIDE_ITEM, c.V)
    ctx.gramian(fh.SIDE_ITEM, fetch=False)
    return ctx


def _loss_rows(got, ref, what, **kw):
    live = ref != 0
    err = np.abs(got[live] - ref[live]) / np.abs(ref[live])
    worst = np.nonzero(live)[0][int(np.argmax(err))]
    print(f"aux loss {what}: worst row {err.max():.2e} at row {worst}")
    report(test="aux", entry="user_loss", what=what, err=float(err.max()), bar=LOSS_TOL,
           margin=LOSS_TOL / max(float(err.max()), 1e-30), worst_row=int(worst), **kw)
    assert err.max() <= LOSS_TOL, (what, float(err.max()), int(worst))
    assert np.all(got[~live] == 0.0), (what, np.nonzero(~live & (got != 0))[0], got[~live])


@pytest.mark.parametrize("dim", LOSS_DIMS)
@pytest.mark.parametrize("beta,half", list(itertools.product((0.0, 0.005), (False, True))))
def test_user_loss_vs_float64(dim, beta, half):
    assert {fh.padded_dim(d) for d in LOSS_DIMS} == set(QUAD_PATH)
    c = _loss_case(dim)
    with _loss_ctx(c, dim) as ctx:
        got = ctx.user_loss(fh.SIDE_USER, beta, half)
    ref = _loss_ref(c, fh.SIDE_USER, beta, half)
    assert tuple(np.nonzero(ref == 0)[0]) == A.IDLE
    _loss_rows(got, ref, f"user d={dim} beta={beta} half={half}", dim=dim, beta=beta, half=half)


@pytest.mark.parametrize("dim", LOSS_DIMS)
def test_user_loss_eval_side(dim):
    c = _loss_case(dim)
    with _loss_ctx(c, dim) as ctx:
        ctx.load_csr(fh.SIDE_EVAL, c.ep, c.ec)
        ctx.set_embeddings(fh.SIDE_EVAL, c.Ue)
        ctx.gramian(fh.SIDE_ITEM, fetch=False)
        for beta, half in ((0.005, True), (0.0, False)):
            got = ctx.user_loss(fh.SIDE_EVAL, beta, half)
            ref = _loss_ref(c, fh.SIDE_EVAL, beta, half)
            assert got.shape == (A.EVAL_ROWS,) and ref[0] != 0 and ref[60] == 0
            _loss_rows(got, ref, f"eval d={dim} beta={beta} half={half}", dim=dim, beta=beta,
                       half=half)


@pytest.mark.parametrize("dim", LOSS_DIMS)
def test_user_loss_after_eval_loss(dim):
    """USER, EVAL, USER on one context: the third call is the first one again,
    idle users (two of them below the 70 EVAL rows) included."""
    c = _loss_case(dim)
    with _loss_ctx(c, dim) as ctx:
        ctx.load_csr(fh.SIDE_EVAL, c.ep, c.ec)
        ctx.set_embeddings(fh.SIDE_EVAL, c.Ue)
        ctx.gramian(fh.SIDE_ITEM, fetch=False)
        first = ctx.user_loss(fh.SIDE_USER, 0.005, True)
        ev = ctx.user_loss(fh.SIDE_EVAL, 0.005, True)
        third = ctx.user_loss(fh.SIDE_USER, 0.005, True)
    assert ev[0] != 0 and ev[61] != 0  # what would show through at users 0 and 61
    _loss_rows(first, _loss_ref(c, fh.SIDE_USER, 0.005, True), f"first of three d={dim}", dim=dim)
    assert np.all(third[list(A.IDLE)] == 0.0), third[list(A.IDLE)]
    np.testing.assert_array_equal(third, first)


@pytest.mark.parametrize("dim", LOSS_DIMS)
def test_user_loss_after_csr_reload(dim):
    """A second load_csr(SIDE_USER) that empties user 1's history: row 1 reads
    0, not the loss of its earlier history."""
    c = _loss_case(dim)
    assert c.up[2] - c.up[1] == 1
    up2 = np.concatenate([c.up[:2], c.up[2:] - 1])
    uc2 = np.delete(c.uc, c.up[1])
    with _loss_ctx(c, dim) as ctx:
        before = ctx.user_loss(fh.SIDE_USER, 0.0, False)
        ctx.load_csr(fh.SIDE_USER, up2, uc2)
        ctx.gramian(fh.SIDE_ITEM, fetch=False)
        after = ctx.user_loss(fh.SIDE_USER, 0.0, False)
    ref = np.array(_loss_ref(c, fh.SIDE_USER, 0.0, False))
    assert before[1] != 0 and ref[1] != 0
    ref[1] = 0.0
    _loss_rows(after, ref, f"reload d={dim}", dim=dim)
    assert after[1] == 0.0
    keep = np.arange(c.nu) != 1
    np.testing.assert_array_equal(after[keep], before[keep])


# ---------------------------------------------------------------- train stats, residual
def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))


@pytest.mark.parametrize("dim", [8, 64, 256, 500])
def test_train_stats_vs_float64(dim):
    c = _loss_case(dim)
    with _loss_ctx(c, dim) as ctx:
        obs, unobs, un, vn = ctx.train_stats()
    r_obs, r_unobs, r_un, r_vn = R.train_stats64(c.up, c.uc, c.U, c.V)
    e = dict(observed=_rel(obs, r_obs), unobserved=_rel(unobs, r_unobs), user_norm2=_rel(un, r_un),
             item_norm2=_rel(vn, r_vn))
    print(f"aux train_stats d={dim}: {e}")
    worst = max(e.values())
    report(test="aux", entry="train_stats", dim=dim, err=worst, bar=STATS_TOL,
           margin=STATS_TOL / max(worst, 1e-30), **e)
    for k, v in e.items():
        assert v <= STATS_TOL, (k, v)


@pytest.mark.parametrize("dim", [8, 100, 1000])
@pytest.mark.parametrize("n", [1, 5, 121])
def test_snapshot_residual_vs_float64(dim, n):
    rng = np.random.default_rng(100 * dim + n)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Y = X.copy()
    Y[::3] += (0.05 * rng.standard_normal(Y[::3].shape)).astype(np.float32)
    with fh.Context(dim, n, 1) as ctx:
        ctx.set_embeddings(fh.SIDE_USER, X)
        ctx.snapshot(fh.SIDE_USER)
        zero = ctx.snapshot_residual(fh.SIDE_USER)
        ctx.set_embeddings(fh.SIDE_USER, Y)
        got = ctx.snapshot_residual(fh.SIDE_USER)
    ref = float(np.sum((Y.astype(np.float64) - X.astype(np.float64)) ** 2))
    e = abs(got - ref) / ref
    print(f"aux snapshot_residual d={dim} n={n}: {e:.2e}")
    report(test="aux", entry="snapshot_residual", dim=dim, rows=n, err=e, bar=STATS_TOL,
           margin=STATS_TOL / max(e, 1e-30))
    assert zero == 0.0
    assert e <= STATS_TOL, e
