"""History-space ("dual") solve path: the basis change G = Q T Q^T and the
h x h push-through solve (dual.hip, spectral.hip) against the d-space solve
and the CPU oracle.  The parity bar is the same as test_parity_gpu.py's
(1e-4 relative per row); FRECSYS_DUAL=0 forces the d-space kernel for every
entity, FRECSYS_DUAL_MAX_H moves the split between the two paths.
"""
import os

import numpy as np
import pytest

import numpy_ref as R
import oracle as O
from conftest import rel_rows
from test_models_gpu import report
from test_parity_gpu import _ctx, _v_inputs, _weights

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

TOL_ROW = 1e-4


def _spread_embeddings(n, dim, seed):
    """Rows with a wide, partly clustered spectrum (trained-model-like)."""
    rng = np.random.default_rng(seed)
    scales = np.geomspace(1.0, 0.03, dim)
    scales[dim // 3: dim // 3 + 8] = 0.5  # a cluster of equal eigenvalues
    return (rng.standard_normal((n, dim)) * scales).astype(np.float32)


@pytest.mark.parametrize("dim", [64, 50, 96, 128, 200, 256])
def test_basis_orthogonal_and_exact(quirk_data, dim):
    nu, ni, up, uc, ip, ic = quirk_data
    ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
    ctx.set_embeddings(fh.SIDE_USER, _spread_embeddings(nu, dim, 4))
    G = ctx.gramian(fh.SIDE_USER).astype(np.float64)
    Q, dg, sb = ctx.debug_basis(fh.SIDE_USER)
    Dp = fh.padded_dim(dim)
    Q = Q.astype(np.float64)
    assert np.abs(Q.T @ Q - np.eye(Dp)).max() < 2e-6
    T = np.diag(dg.astype(np.float64)) + np.diag(sb[:-1].astype(np.float64), -1) \
        + np.diag(sb[:-1].astype(np.float64), 1)
    Gp = np.zeros((Dp, Dp))
    Gp[:dim, :dim] = G
    err = np.abs(Q @ T @ Q.T - Gp).max() / np.abs(Gp).max()
    assert err < 5e-6, err
    # padded coordinates stay out of the basis: Q = diag(Q1, I)
    if Dp > dim:
        np.testing.assert_array_equal(Q[dim:, :dim], 0.0)
        np.testing.assert_array_equal(Q[dim:, dim:], np.eye(Dp - dim))
    assert sb[-1] == 0.0


def _both_paths(monkeypatch, make, max_h=None):
    outs = []
    for on in ("0", "1"):
        monkeypatch.setenv("FRECSYS_DUAL", on)
        if max_h is not None:
            monkeypatch.setenv("FRECSYS_DUAL_MAX_H", str(max_h))
        outs.append(make())
    return outs


@pytest.mark.parametrize("dim", [64, 96, 128, 256])
@pytest.mark.parametrize("max_h", [256, 64])
@pytest.mark.parametrize("reg_exp", [1.0, 0.0])
def test_ials_dual_vs_dspace_vs_oracle(monkeypatch, quirk_data, dim, max_h, reg_exp):
    """iALS with the default l2_reg_exp = 1 (lambda per user: the tridiagonal
    basis) and with l2_reg_exp = 0 (one M = w G + reg I for every user: the
    Cholesky basis)."""
    nu, ni, up, uc, ip, ic = quirk_data
    reg, w = 0.003, 0.1
    V0 = _spread_embeddings(ni, dim, 8)
    basis = "chol" if reg_exp == 0.0 else "tridiag"

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
        ctx.set_embeddings(fh.SIDE_ITEM, V0)
        ctx.gramian(fh.SIDE_ITEM)
        ctx.timing_reset()
        ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, reg, w, reg_exp=reg_exp)
        hs = ctx.timing("solve_user.hspace")[1]
        if hs:
            assert ctx.work("basis_chol")[2] == (basis == "chol")
            assert ctx.work("basis_tridiag")[2] == (basis == "tridiag")
        return ctx.get_embeddings(fh.SIDE_USER), U, hs

    (Ud, U, hs0), (Uh, _, hs1) = _both_paths(monkeypatch, run, max_h)
    assert hs0 == 0 and hs1 == 1  # the split really happened
    Uo, rc = O.step(up, uc, V0, O.gramian(V0), 0, reg, w, reg_exp=reg_exp, out=U.copy())
    assert rc == 0
    assert rel_rows(Ud, Uo).max() < TOL_ROW
    assert rel_rows(Uh, Uo).max() < TOL_ROW
    np.testing.assert_array_equal(Uh[5], U[5])  # idle user untouched
    h = np.diff(up)
    long = h > max_h
    np.testing.assert_array_equal(Uh[long], Ud[long])  # same kernel for the long ones


@pytest.mark.parametrize("dim", [128, 256, 512])
@pytest.mark.parametrize("reg,w", [(0.003, 0.1), (1e-5, 1.0)])
def test_chol_basis_conditioning(monkeypatch, quirk_data, dim, reg, w):
    """iALS with l2_reg_exp = 0: the Cholesky basis against the tridiagonal
    one (FRECSYS_CHOL_BASIS=0) and the oracle on a wide spectrum, including an ill-conditioned M (reg 1e-5, w 1: cond(M)
    ~ 1e8): the explicit L^-T may not lose more than the tridiagonal LDL
    chains do."""
    nu, ni, up, uc, ip, ic = quirk_data
    V0 = _spread_embeddings(ni, dim, 12)
    monkeypatch.setenv("FRECSYS_DUAL", "1")
    monkeypatch.setenv("FRECSYS_DUAL_MAX_H", "256")
    outs = []
    for on in ("1", "0"):
        monkeypatch.setenv("FRECSYS_CHOL_BASIS", on)
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
        ctx.set_embeddings(fh.SIDE_ITEM, V0)
        ctx.gramian(fh.SIDE_ITEM)
        ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, reg, w, reg_exp=0.0)
        assert ctx.work("basis_chol")[2] == (on == "1")
        outs.append(ctx.get_embeddings(fh.SIDE_USER))
        ctx.close()
    G0 = O.gramian(V0)
    Uo, rc = O.step(up, uc, V0, G0, 0, reg, w, reg_exp=0.0, out=U.copy())
    assert rc == 0
    h = np.diff(up)
    hs = (h > 0) & (h <= 256)
    e_chol = rel_rows(outs[0][hs], Uo[hs]).max()
    e_tri = rel_rows(outs[1][hs], Uo[hs]).max()
    # every path against the float64 solution of the same (fp32-rounded)
    # inputs: on the quirk fixture's 400 items G is singular at d = 512
    # (rank <= 400), so with lambda = reg alone cond(A) reaches ~1e4 - 1e8 and
    # two fp32 computations differ by cond x eps whatever their order; the bar
    # there is accuracy -- each GPU basis no worse than the oracle's own fp32
    # restatement of the reference -- and the 1e-4 oracle bar where the
    # conditioning allows it
    rows = np.nonzero(hs)[0]
    X64 = np.array([R.ials(uc[up[r]:up[r + 1]], V0, G0, reg, w) for r in rows])
    f_or = rel_rows(Uo[rows], X64).max()
    f_chol = rel_rows(outs[0][rows], X64).max()
    f_tri = rel_rows(outs[1][rows], X64).max()
    print(f"dim {dim} reg {reg} w {w}: vs oracle chol {e_chol:.2e} tridiag {e_tri:.2e}; "
          f"vs float64 oracle {f_or:.2e} chol {f_chol:.2e} tridiag {f_tri:.2e}")
    report(test="chol_basis_conditioning", dim=dim, reg=reg, w=w, chol=float(e_chol),
           tridiag=float(e_tri), f64_oracle=float(f_or), f64_chol=float(f_chol),
           f64_tridiag=float(f_tri))
    assert f_chol <= max(TOL_ROW, 2.0 * f_or), (f_chol, f_or)
    # the tridiagonal basis is the one every benchmarked config uses
    assert f_tri <= max(TOL_ROW, 2.0 * f_or), (f_tri, f_or)
    if f_or < 1e-5:  # well conditioned: the row bar against the oracle itself
        assert e_chol < TOL_ROW and e_tri < TOL_ROW, (e_chol, e_tri)


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_weighted_u_dual(monkeypatch, quirk_data, dim):
    nu, ni, up, uc, ip, ic = quirk_data
    om = _weights(nu)
    om[::7] = 0.0  # zero dual weights: the row must come out exactly 0
    reg, w = 0.004, 0.004
    V0 = _spread_embeddings(ni, dim, 9)

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
        ctx.set_embeddings(fh.SIDE_ITEM, V0)
        ctx.gramian(fh.SIDE_ITEM)
        ctx.solve_side(fh.SIDE_USER, fh.KIND_WEIGHTED_U, reg, w, entity_weight=om)
        return ctx.get_embeddings(fh.SIDE_USER), U

    (Ud, U), (Uh, _) = _both_paths(monkeypatch, run)
    Uo, rc = O.step(up, uc, V0, O.gramian(V0), 1, reg, w, entity_weight=om, out=U.copy())
    assert rc == 0
    assert rel_rows(Uh, Uo).max() < TOL_ROW
    assert rel_rows(Ud, Uo).max() < TOL_ROW
    zero = (om == 0) & (np.diff(up) > 0)
    assert np.abs(Uh[zero]).max() == 0.0


@pytest.mark.parametrize("dim", [64, 160, 256])
@pytest.mark.parametrize("quirk", [True, False])
def test_weighted_v_dual(monkeypatch, quirk_data, dim, quirk):
    nu, ni, up, uc, ip, ic = quirk_data
    om = _weights(nu)
    om[::5] = 0.0  # users with zero weight contribute nothing (CVaR-style)
    nu_w, item_reg = _v_inputs(nu, ni, up, ip, ic, om)
    reg, w, alpha = 0.004, 0.004, 0.3
    U0 = _spread_embeddings(nu, dim, 10)

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic, quirks=quirk)
        ctx.set_embeddings(fh.SIDE_USER, U0)
        ctx.gramian(fh.SIDE_USER, weights=om)
        ctx.solve_side(fh.SIDE_ITEM, fh.KIND_WEIGHTED_V, reg, w, alpha=alpha,
                       entity_reg=item_reg, other_weight=nu_w)
        return ctx.get_embeddings(fh.SIDE_ITEM), V

    (Vd, V), (Vh, _) = _both_paths(monkeypatch, run)
    Vo, rc = O.step(ip, ic, U0, O.gramian(U0, om), 2, reg, w, alpha=alpha, quirk=int(quirk),
                    entity_reg=item_reg, other_weight=nu_w, out=V.copy())
    assert rc == 0
    assert rel_rows(Vh, Vo).max() < TOL_ROW
    assert rel_rows(Vd, Vo).max() < TOL_ROW


def test_tail_quirk_in_history_space(monkeypatch, quirk_data):
    """Quirk rows (A only, not b) must matter in the history-space form too."""
    nu, ni, up, uc, ip, ic = quirk_data
    monkeypatch.setenv("FRECSYS_DUAL", "1")
    monkeypatch.setenv("FRECSYS_DUAL_MAX_H", "256")  # h_eff = 256 rows in history space
    dim = 64
    om = _weights(nu)
    nu_w, item_reg = _v_inputs(nu, ni, up, ip, ic, om)
    outs = []
    for q in (True, False):
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic, quirks=q)
        ctx.gramian(fh.SIDE_USER, weights=om)
        ctx.solve_side(fh.SIDE_ITEM, fh.KIND_WEIGHTED_V, 0.004, 0.004, alpha=0.3,
                       entity_reg=item_reg, other_weight=nu_w)
        outs.append(ctx.get_embeddings(fh.SIDE_ITEM))
    h = np.diff(ip)
    affected = (h > 128) & (h % 128 != 0) & (h + 128 - h % 128 <= 256)
    assert affected.sum() >= 2
    diff = np.abs(outs[0] - outs[1]).max(axis=1)
    assert (diff[affected] > 0).all()
    np.testing.assert_array_equal(outs[0][h <= 128], outs[1][h <= 128])


def test_eval_side_dual(monkeypatch, ml1m):
    monkeypatch.setenv("FRECSYS_DUAL", "1")
    tr, vt, ve = ml1m
    nu, ni = tr.max_user + 1, tr.max_item + 1
    up, uc = tr.by_user()
    ip, ic = tr.by_item()
    ctx, U, V = _ctx(128, nu, ni, up, uc, ip, ic)
    V0 = _spread_embeddings(ni, 128, 11)
    ctx.set_embeddings(fh.SIDE_ITEM, V0)
    ids, ep, ec = vt.compact_users()
    ctx.load_csr(fh.SIDE_EVAL, ep, ec)
    ctx.gramian(fh.SIDE_ITEM)
    ctx.solve_side(fh.SIDE_EVAL, fh.KIND_IALS, 0.003, 0.1)
    Uo, rc = O.step(ep, ec, V0, O.gramian(V0), 0, 0.003, 0.1)
    assert rel_rows(ctx.get_embeddings(fh.SIDE_EVAL), Uo).max() < TOL_ROW


def _buckets(h):
    """History-space bucket t (32 (t-1) < h <= 32 t) per entity, as the host
    queue split in train.hip plan_side assigns them (iALS: h_eff = h)."""
    b = np.ceil(np.asarray(h) / 32.0).astype(int)
    return [int(((b == t) & (np.asarray(h) > 0)).sum()) for t in range(1, 9)]


def test_every_bucket_filled_and_solved(quirk_data, monkeypatch):
    """The default fixture puts entities in every history-space bucket
    TH = 1..8 on both sides (TH = 6 and 8 run the MFMA-blocked diagonal
    factor, TH <= 2 the wave-per-entity kernel) and some in d space; one
    iALS epoch over it matches the oracle on every row."""
    nu, ni, up, uc, ip, ic = quirk_data
    hu, hi = np.diff(up), np.diff(ip)
    assert all(c > 0 for c in _buckets(hu)), _buckets(hu)
    assert all(c > 0 for c in _buckets(hi)), _buckets(hi)
    assert (hu > 256).any() and (hi > 256).any()
    dim = 256
    monkeypatch.setenv("FRECSYS_DUAL_MAX_H", "256")  # TH = 8 too (the d=256 default is 224)
    ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
    assert ctx.history_space_max_h() == 256
    reg, w = 0.003, 0.1
    ctx.gramian(fh.SIDE_ITEM)
    ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, reg, w)
    assert ctx.timing("solve_user.hspace")[1] == 1 and ctx.timing("solve_user.dspace")[1] == 1
    Uo, rc = O.step(up, uc, V, O.gramian(V), 0, reg, w, out=U.copy())
    assert rc == 0
    assert rel_rows(ctx.get_embeddings(fh.SIDE_USER), Uo).max() < TOL_ROW
    ctx.set_embeddings(fh.SIDE_USER, Uo)
    ctx.gramian(fh.SIDE_USER)
    ctx.solve_side(fh.SIDE_ITEM, fh.KIND_IALS, reg, w)
    assert ctx.timing("solve_item.hspace")[1] == 1 and ctx.timing("solve_item.dspace")[1] == 1
    Vo, rc = O.step(ip, ic, Uo, O.gramian(Uo), 0, reg, w, out=V.copy())
    assert rc == 0
    assert rel_rows(ctx.get_embeddings(fh.SIDE_ITEM), Vo).max() < TOL_ROW


@pytest.mark.parametrize("dim,expect,user", [(32, 0, 0), (64, 224, 224), (256, 224, 224),
                                              (512, 256, 320), (1024, 512, 512)])
def test_default_history_space_threshold(quirk_data, dim, expect, user):
    """Crossover of the two paths (capi.hip): h_eff <= 224 at Dp <= 256 (the
    d-space kernel is faster for the TH = 8 bucket there), 256 at Dp = 512
    (the user side 320: its half-step is d-space bound), 512 at
    Dp = 1024 (the wide bucket, dual.hip); no history-space path below
    Dp = 64."""
    nu, ni, up, uc, ip, ic = quirk_data
    ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
    assert ctx.history_space_max_h() == expect
    assert ctx.history_space_max_h(fh.SIDE_USER) == user
    assert ctx.history_space_max_h(fh.SIDE_ITEM) == expect
    ctx.close()


@pytest.mark.parametrize("dim", [512, 1024])
@pytest.mark.parametrize("side", ["user", "item"])
def test_wide_trained_spectrum_half_step(monkeypatch, quirk_data, dim, side):
    """d = 512 / 1024 on a trained-model-like spectrum (wide, partly
    clustered eigenvalues of G) rather than isotropic random rows: the
    tridiagonal history-space path (h <= 256, iALS l2_reg_exp = 1 -- the
    benchmark configuration) and the wide d-space path (h > 256; and every
    entity with FRECSYS_DUAL=0) against the oracle, every row at the bar."""
    nu, ni, up, uc, ip, ic = quirk_data
    reg, w = 0.003, 0.1
    if side == "user":
        s, o, ptr, col, n_o = fh.SIDE_USER, fh.SIDE_ITEM, up, uc, ni
    else:
        s, o, ptr, col, n_o = fh.SIDE_ITEM, fh.SIDE_USER, ip, ic, nu
    X0 = _spread_embeddings(n_o, dim, 21 + dim)

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
        ctx.set_embeddings(o, X0)
        ctx.gramian(o)
        ctx.timing_reset()
        ctx.solve_side(s, fh.KIND_IALS, reg, w)
        hs = ctx.timing(("solve_user" if side == "user" else "solve_item") + ".hspace")[1]
        if hs:
            assert ctx.work("basis_tridiag")[2] == 1
        assert ctx.counter("hspace_reruns") == 0
        out = ctx.get_embeddings(s)
        ctx.close()
        return out, (U if side == "user" else V), hs

    (Xd, X, hs0), (Xh, _, hs1) = _both_paths(monkeypatch, run)
    assert hs0 == 0 and hs1 == 1
    Xo, rc = O.step(ptr, col, X0, O.gramian(X0), 0, reg, w, out=X.copy())
    assert rc == 0
    h = np.diff(ptr)
    e_d, e_h = rel_rows(Xd, Xo), rel_rows(Xh, Xo)
    short = (h > 0) & (h <= 256)
    # attribution: the worst rows of each path against the float64 solution
    # of the same fp32 inputs, beside the oracle's own fp32 error there (the
    # quirk fixture has 300 items: at d = 1024 the user side's G has rank
    # <= 300 and M = w G + lambda I is conditioned by lambda alone)
    rows = np.unique(np.concatenate([np.argsort(e_d)[-24:], np.argsort(e_h)[-24:]]))
    rows = rows[h[rows] > 0]
    G0 = O.gramian(X0)
    # lambda = reg (h + w n_other)^l2_reg_exp, l2_reg_exp = 1, in fp32 as the
    # product forms it (ials.h:310-315)
    lam = np.float32(reg) * (h[rows].astype(np.float32) + np.float32(w) * np.float32(n_o))
    X64 = np.array([R.ials(col[ptr[r]:ptr[r + 1]], X0, G0, l, w) for r, l in zip(rows, lam)])
    f_or = rel_rows(Xo[rows], X64).max()
    f_d = rel_rows(Xd[rows], X64).max()
    f_h = rel_rows(Xh[rows], X64).max()
    report(test="wide_trained_spectrum", side=side, dim=dim,
           dspace_max=float(e_d.max()), hspace_max=float(e_h[short].max()),
           split_dspace_max=float(e_h[h > 256].max()) if (h > 256).any() else None,
           f64_oracle=float(f_or), f64_dspace=float(f_d), f64_hspace=float(f_h),
           env={k: v for k, v in os.environ.items() if k.startswith("FRECSYS_")})
    print(f"{side} d={dim}: vs oracle dspace {e_d.max():.2e} hspace {e_h.max():.2e}; vs float64 "
          f"(worst rows) oracle {f_or:.2e} dspace {f_d:.2e} hspace {f_h:.2e}")
    assert e_d.max() < TOL_ROW, e_d.max()
    assert e_h.max() < TOL_ROW, e_h.max()
