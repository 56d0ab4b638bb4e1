"""The dataflow Cholesky's static worker schedule (csrc/chol_sched.h, chol.h
chol_solve_df) against the round-robin order it replaces: FRECSYS_CHOL_SCHED
= 1 (the default) and = 0 run the same tasks with the same arithmetic in
another order on other waves, so every solved row is the same bits.  The
table is the (T, NW) = (8, 8) one: d space at Dp = 256 and the history-space
bucket TH = 8 walk it; Dp = 224 (T = 7) and the other buckets have none and
must not be touched by the switch.
"""
import numpy as np
import pytest

from test_dual_gpu import _buckets, _spread_embeddings
from test_parity_gpu import _ctx, _v_inputs, _weights

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")


def _both_orders(monkeypatch, make):
    outs = []
    for on in ("1", "0"):
        monkeypatch.setenv("FRECSYS_CHOL_SCHED", on)
        outs.append(make())
    return outs


def _same(a, b):
    assert np.isfinite(a).all() and np.isfinite(b).all()
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dim", [256, 224, 200])
@pytest.mark.parametrize("side", ["user", "item"])
def test_dspace_ials(monkeypatch, quirk_data, dim, side):
    nu, ni, up, uc, ip, ic = quirk_data
    monkeypatch.setenv("FRECSYS_DUAL", "0")  # every entity through the d-space kernel
    s, o = (fh.SIDE_USER, fh.SIDE_ITEM) if side == "user" else (fh.SIDE_ITEM, fh.SIDE_USER)
    X0 = _spread_embeddings(ni if side == "user" else nu, dim, 8)

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
        ctx.set_embeddings(o, X0)
        ctx.gramian(o)
        ctx.timing_reset()
        ctx.solve_side(s, fh.KIND_IALS, 0.003, 0.1)
        assert ctx.timing(f"solve_{side}.hspace")[1] == 0
        return ctx.get_embeddings(s)

    a, b = _both_orders(monkeypatch, run)
    _same(a, b)


@pytest.mark.parametrize("dim", [256, 224, 200])
def test_dspace_weighted_u(monkeypatch, quirk_data, dim):
    nu, ni, up, uc, ip, ic = quirk_data
    monkeypatch.setenv("FRECSYS_DUAL", "0")
    om = _weights(nu)
    om[::7] = 0.0
    V0 = _spread_embeddings(ni, dim, 9)

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
        ctx.set_embeddings(fh.SIDE_ITEM, V0)
        ctx.gramian(fh.SIDE_ITEM)
        ctx.solve_side(fh.SIDE_USER, fh.KIND_WEIGHTED_U, 0.004, 0.004, entity_weight=om)
        return ctx.get_embeddings(fh.SIDE_USER)

    a, b = _both_orders(monkeypatch, run)
    _same(a, b)


@pytest.fixture(scope="module")
def v_inputs(quirk_data):
    nu, ni, up, uc, ip, ic = quirk_data
    om = _weights(nu)
    om[::5] = 0.0
    return (om,) + _v_inputs(nu, ni, up, ip, ic, om)


@pytest.mark.parametrize("dim", [256, 224, 200])
@pytest.mark.parametrize("quirk", [True, False])
def test_dspace_weighted_v(monkeypatch, quirk_data, v_inputs, dim, quirk):
    nu, ni, up, uc, ip, ic = quirk_data
    monkeypatch.setenv("FRECSYS_DUAL", "0")
    om, nu_w, item_reg = v_inputs
    U0 = _spread_embeddings(nu, dim, 10)

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic, quirks=quirk)
        ctx.set_embeddings(fh.SIDE_USER, U0)
        ctx.gramian(fh.SIDE_USER, weights=om)
        ctx.solve_side(fh.SIDE_ITEM, fh.KIND_WEIGHTED_V, 0.004, 0.004, alpha=0.3,
                       entity_reg=item_reg, other_weight=nu_w)
        return ctx.get_embeddings(fh.SIDE_ITEM)

    a, b = _both_orders(monkeypatch, run)
    _same(a, b)


def test_history_space_every_bucket(monkeypatch, quirk_data):
    """TH = 1..8 all filled on both sides: the TH = 8 bucket walks the table,
    the others (TH = 7 among them) keep their loops."""
    nu, ni, up, uc, ip, ic = quirk_data
    assert all(c > 0 for c in _buckets(np.diff(up))) and all(c > 0 for c in _buckets(np.diff(ip)))
    monkeypatch.setenv("FRECSYS_DUAL", "1")
    monkeypatch.setenv("FRECSYS_DUAL_MAX_H", "256")
    dim = 256
    U0 = _spread_embeddings(nu, dim, 12)
    V0 = _spread_embeddings(ni, dim, 13)

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
        assert ctx.history_space_max_h() == 256
        ctx.set_embeddings(fh.SIDE_USER, U0)
        ctx.set_embeddings(fh.SIDE_ITEM, V0)
        ctx.gramian(fh.SIDE_ITEM)
        ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, 0.003, 0.1)
        assert ctx.timing("solve_user.hspace")[1] == 1
        Un = ctx.get_embeddings(fh.SIDE_USER)
        ctx.set_embeddings(fh.SIDE_USER, U0)
        ctx.gramian(fh.SIDE_USER)
        ctx.solve_side(fh.SIDE_ITEM, fh.KIND_IALS, 0.003, 0.1)
        assert ctx.timing("solve_item.hspace")[1] == 1
        return Un, ctx.get_embeddings(fh.SIDE_ITEM)

    (Ua, Va), (Ub, Vb) = _both_orders(monkeypatch, run)
    _same(Ua, Ub)
    _same(Va, Vb)


def test_two_epoch_trajectory(monkeypatch, quirk_data):
    """Two iALS epochs at d = 256 with the default split of the two paths."""
    nu, ni, up, uc, ip, ic = quirk_data

    def run():
        ctx, U, V = _ctx(256, nu, ni, up, uc, ip, ic)
        for _ in range(2):
            ctx.gramian(fh.SIDE_ITEM, fetch=False)
            ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, 0.003, 0.1)
            ctx.gramian(fh.SIDE_USER, fetch=False)
            ctx.solve_side(fh.SIDE_ITEM, fh.KIND_IALS, 0.003, 0.1)
        return ctx.get_embeddings(fh.SIDE_USER), ctx.get_embeddings(fh.SIDE_ITEM)

    (Ua, Va), (Ub, Vb) = _both_orders(monkeypatch, run)
    _same(Ua, Ub)
    _same(Va, Vb)


@pytest.mark.parametrize("dim", [256, 224])
def test_failing_entity_reported_the_same(monkeypatch, quirk_data, v_inputs, dim):
    """One item's regulariser made hugely negative: its matrix alone is not
    SPD, and both orders name that item."""
    nu, ni, up, uc, ip, ic = quirk_data
    monkeypatch.setenv("FRECSYS_DUAL", "0")
    om, nu_w, item_reg = v_inputs
    bad = int(np.argmax(np.diff(ip) > 0)) + 37
    assert ip[bad + 1] > ip[bad]
    reg_bad = item_reg.copy()
    reg_bad[bad] = -1e7

    def run():
        ctx, U, V = _ctx(dim, nu, ni, up, uc, ip, ic)
        ctx.gramian(fh.SIDE_USER, weights=om)
        with pytest.raises(fh.FrecsysError) as ei:
            ctx.solve_side(fh.SIDE_ITEM, fh.KIND_WEIGHTED_V, 0.004, 0.004, alpha=0.3,
                           entity_reg=reg_bad, other_weight=nu_w)
        assert ei.value.code == fh.ERR_NOT_SPD
        return ei.value.entity

    a, b = _both_orders(monkeypatch, run)
    assert a == b == bad
