"""The iALS++ / SAFER2++ block step (csrc/pp.hip: pp_block_kernel<TB>,
pp_predict_kernel, pp_refresh_kernel; frecsys_pp_* in train.hip) at its seams
against float64.

One block step per case of tests/pp_ref.py on the seam fixture: every TB at
its lower and upper width and one column on either side of every 32-column
tile, unaligned starts, blocks ending at dim with and without padding behind
them, Dp up to 1024, history lengths on the 32-row staging seam, repeated
ids, omega = 0 entities and nu = 0 rows.  The new block and the entity's
predictions are compared with the float64 restatement in the two measures of
pp_ref.py -- not with the fp32 oracle, whose own error in the same measures
test_pp_seam_cpu.py caps at a quarter of the bar -- the residual with the
float64 one, and everything outside the block bit for bit with the start.

Then: pp_predict alone under its dot-product bound, the EVAL side against
the USER side bit for bit, two consecutive blocks, the sharded refresh at the
lane seams of pp_refresh_kernel, and the NOT_SPD verdict of every TB.

The worst block, its history length and the oracle's figures on the same
case go to parity_report.jsonl (test = "pp_seams").
"""
import math
import os

import numpy as np
import pytest

import pp_ref as P
from test_models_gpu import report

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

TOL = 1e-4      # TOL_ROW, the project's row bar
TOL_RESID = 1e-4

_slot = {}  # the one live context: (key, dim) -> Context


@pytest.fixture(scope="module", autouse=True)
def _close_last_context():
    yield
    if "ctx" in _slot:
        _slot.pop("ctx").close()
    _slot.clear()


def _drop_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("FRECSYS_")]:
        monkeypatch.delenv(k)


def _make(c, p, world=1, rank=0):
    ctx = fh.Context(c.dim, c.nu, c.ni, parity_quirks=c.quirk)
    if world > 1:
        ctx.comm_init(world, rank, None)
    ctx.load_csr(fh.SIDE_USER, c.up, c.uc)
    ctx.load_csr(fh.SIDE_ITEM, c.ip, c.ic)
    ctx.pp_set_rating_index(fh.SIDE_USER, p.urix)
    ctx.pp_set_rating_index(fh.SIDE_ITEM, p.irix)
    return ctx


def _context(monkeypatch, key, dim):
    """The context of case (key, dim), made once; a new case closes the last."""
    _drop_env(monkeypatch)
    p = P.pp_case(key, dim)
    if _slot.get("case") != (key, dim):
        if "ctx" in _slot:
            _slot.pop("ctx").close()
        _slot["ctx"] = _make(p.c, p)
        _slot["case"] = (key, dim)
    assert fh.padded_dim(dim) == P.PADDED[dim]
    return _slot["ctx"], p


def _sides(c):
    return (fh.SIDE_USER, fh.SIDE_ITEM) if c.seam == "user" else (fh.SIDE_ITEM, fh.SIDE_USER)


def _reset(ctx, c):
    """Both tables back to the start rows, the predictions of them, and the
    Gramian of the other side."""
    ctx.set_embeddings(fh.SIDE_USER, c.U)
    ctx.set_embeddings(fh.SIDE_ITEM, c.V)
    ctx.pp_predict(fh.SIDE_USER)
    ctx.gramian(_sides(c)[1], weights=c.gram_weights, fetch=False)


def _step_kw(c):
    if c.kind == fh.KIND_IALS:
        return dict(reg_exp=c.reg_exp)
    if c.kind == fh.KIND_WEIGHTED_U:
        return dict(kind=c.kind, entity_weight=c.entity_weight)
    return dict(kind=c.kind, alpha=c.alpha, entity_reg=c.entity_reg, other_weight=c.other_weight)


def _step(ctx, c, s, e, side=None, reg=None):
    return ctx.pp_step(_sides(c)[0] if side is None else side, s, e,
                       c.reg if reg is None else reg, c.w, **_step_kw(c))


def _read(ctx, c, p):
    side, other = _sides(c)
    return (ctx.get_embeddings(side), ctx.get_embeddings(other),
            ctx.pp_predictions(fh.SIDE_USER, p.nnz))


def _against_float64(p, ref, E, pred, resid, what):
    """The 1e-4 measures of one step; returns the figures for the report."""
    c = p.c
    assert sum(int(c.h[e]) for e in p.live) == p.nnz == len(pred)  # every entry is measured
    eb, ep = P.block_errors(p, ref, E), P.pred_errors(p, ref, pred)
    er = abs(resid - ref.residual) / ref.residual
    wb, wp = P.worst(p, eb), P.worst(p, ep)
    print(f"pp_seams {what}: block {wb[0]:.2e} (h = {wb[1]}, {wb[2]}) pred {wp[0]:.2e} "
          f"(h = {wp[1]}, {wp[2]}) residual {er:.2e}")
    bad_b, bad_p = P.offenders(p, eb, TOL), P.offenders(p, ep, TOL)
    assert not bad_b, f"{what}: blocks (h, label, error) past {TOL}: {bad_b}"
    assert not bad_p, f"{what}: predictions (h, label, error) past {TOL}: {bad_p}"
    assert er <= TOL_RESID, (what, resid, ref.residual)
    return wb, wp, er


def _untouched_outside(c, s, e, E, other, E0=None):
    """Bitwise the start: the columns outside [s, e) (those a caller can read,
    up to dim), idle rows, the other side."""
    E0 = c.E if E0 is None else E0
    np.testing.assert_array_equal(E[:, :s], E0[:, :s])
    np.testing.assert_array_equal(E[:, e:], E0[:, e:])
    idle = c.h == 0
    assert idle.sum() >= 3
    np.testing.assert_array_equal(E[idle], E0[idle])
    np.testing.assert_array_equal(other, c.X)


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_block_step_vs_float64(monkeypatch, case):
    key, dim, (s, e) = case
    ctx, p = _context(monkeypatch, key, dim)
    c = p.c
    _reset(ctx, c)
    resid = _step(ctx, c, s, e)
    E, other, pred = _read(ctx, c, p)
    ref, = P.reference(key, dim, (s, e))
    orc, = P.oracle_steps(key, dim, (s, e))
    ob, op = P.worst(p, P.block_errors(p, ref, orc.E)), P.worst(p, P.pred_errors(p, ref, orc.pred))
    eb, ep = P.block_errors(p, ref, E), P.pred_errors(p, ref, pred)
    wb, wp = P.worst(p, eb), P.worst(p, ep)
    er = abs(resid - ref.residual) / ref.residual
    report(test="pp_seams", kind=key, dim=dim, start=s, end=e, tb=P.tile_count(e - s),
           max_block=wb[0], worst_h=wb[1], worst_label=wb[2], max_pred=wp[0], pred_worst_h=wp[1],
           pred_worst_label=wp[2], residual_rel=er, f64_oracle_max_block=ob[0],
           f64_oracle_max_pred=op[0],
           f64_oracle_residual_rel=abs(orc.residual - ref.residual) / ref.residual,
           margin=TOL / max(wb[0], wp[0], 1e-30))
    assert ob[0] < P.ORACLE_CAP and op[0] < P.ORACLE_CAP  # the restatement's own share
    _against_float64(p, ref, E, pred, resid, P.case_id(case))
    _untouched_outside(c, s, e, E, other)
    # the existing bar against the oracle stays where it is
    assert abs(resid - orc.residual) <= 1e-3 * orc.residual + 1e-12


@pytest.mark.parametrize("dim", P.DIMS)
@pytest.mark.parametrize("key", ["ials_user", "ials_item"])
def test_predict_vs_float64(monkeypatch, key, dim):
    """pp_predict_kernel: one product, ceil(Dp / 64) adds per lane and six
    butterfly adds per entry -- the standard dot-product bound of that chain,
    doubled."""
    ctx, p = _context(monkeypatch, key, dim)
    c = p.c
    ctx.set_embeddings(fh.SIDE_USER, c.U)
    ctx.set_embeddings(fh.SIDE_ITEM, c.V)
    ctx.pp_predict(fh.SIDE_USER)
    pred = ctx.pp_predictions(fh.SIDE_USER, p.nnz)
    ref, mag = P.pred0(p), P.pred0_magnitude(p)
    Dp = P.PADDED[dim]
    bound = 2 * (math.ceil(Dp / 64) + 7) * 2.0 ** -24 * mag
    err = np.abs(pred.astype(np.float64) - ref)
    worst = int(np.argmax(err / bound))
    print(f"pp_seams predict {key} d={dim}: worst |err| / bound {err[worst] / bound[worst]:.3f}")
    assert len(pred) == p.nnz and (mag > 0).all()
    assert (err <= bound).all(), (worst, float(err[worst]), float(bound[worst]))


@pytest.mark.parametrize("block", [(35, 100), (67, 100)], ids=["w65", "w33"])
def test_eval_side_is_the_user_side_bitwise(monkeypatch, block):
    """SIDE_EVAL (CSR position as rating index, a prediction vector of its
    own) from the same start rows as a USER step whose rating index is the
    identity: the same bits in the rows, the predictions and the residual."""
    s, e = block
    ctx, p = _context(monkeypatch, "ials_user", 100)
    c = p.c
    np.testing.assert_array_equal(p.urix, np.arange(p.nnz))
    _reset(ctx, c)
    r_user = _step(ctx, c, s, e)
    Eu, Vu, pu = _read(ctx, c, p)
    ctx.load_csr(fh.SIDE_EVAL, c.up, c.uc)
    ctx.set_embeddings(fh.SIDE_EVAL, c.U)
    ctx.pp_predict(fh.SIDE_EVAL)
    r_eval = _step(ctx, c, s, e, side=fh.SIDE_EVAL)
    Ee = ctx.get_embeddings(fh.SIDE_EVAL)
    pe = ctx.pp_predictions(fh.SIDE_EVAL, p.nnz)
    assert (Eu[p.live, s:e] != c.U[p.live, s:e]).any(axis=1).all()  # the step moved every live row
    np.testing.assert_array_equal(Ee, Eu)
    np.testing.assert_array_equal(pe, pu)
    assert r_eval == r_user
    # the EVAL step wrote neither the USER table, nor its predictions, nor the items
    np.testing.assert_array_equal(ctx.get_embeddings(fh.SIDE_USER), Eu)
    np.testing.assert_array_equal(ctx.pp_predictions(fh.SIDE_USER, p.nnz), pu)
    np.testing.assert_array_equal(ctx.get_embeddings(fh.SIDE_ITEM), Vu)


@pytest.mark.parametrize("key", P.TWO_STEP_KEYS)
def test_two_consecutive_blocks(monkeypatch, key):
    """[0,65) then [65,100) at d = 100 against the float64 sequence: the
    second step consumes the predictions the first one left."""
    ctx, p = _context(monkeypatch, key, 100)
    c = p.c
    _reset(ctx, c)
    refs = P.reference(key, 100, P.TWO_STEP)
    before = c.E
    for (s, e), ref in zip(P.TWO_STEP, refs):
        resid = _step(ctx, c, s, e)
        E, other, pred = _read(ctx, c, p)
        _against_float64(p, ref, E, pred, resid, f"{key} two-step [{s},{e})")
        _untouched_outside(c, s, e, E, other, before)
        before = E


@pytest.mark.parametrize("bs", [1, 63, 65, 127])
def test_sharded_refresh_at_the_lane_seams(monkeypatch, bs):
    """World 2 on one device, external exchange: the rows every rank did not
    solve get their predictions from pp_refresh_kernel (one lane per column,
    a second element per lane from width 65).  One user and one item block
    step with pp_sync: rows and predictions of every rank are bitwise the
    single-rank ones."""
    from test_sharded_gpu import _allgather_rows, _allreduce_gram
    _drop_env(monkeypatch)
    p = P.pp_case("ials_user", 200)
    c = p.c
    s, e = 200 - bs - 5, 200 - 5  # an unaligned start
    ctxs = [_make(c, p)] + [_make(c, p, 2, r) for r in range(2)]
    try:
        for x in ctxs:
            x.set_embeddings(fh.SIDE_USER, c.U)
            x.set_embeddings(fh.SIDE_ITEM, c.V)
            x.pp_predict(fh.SIDE_USER)
        one, ranks = ctxs[0], ctxs[1:]
        for side, other in ((fh.SIDE_USER, fh.SIDE_ITEM), (fh.SIDE_ITEM, fh.SIDE_USER)):
            one.gramian(other, fetch=False)
            r_one = one.pp_step(side, s, e, c.reg, c.w)
            _allreduce_gram(ranks, other)
            r_sh = sum(x.pp_step(side, s, e, c.reg, c.w) for x in ranks)
            _allgather_rows(ranks, side)
            for x in ranks:
                x.pp_sync(side)
            assert abs(r_sh - r_one) <= 1e-9 * r_one
            want = (one.get_embeddings(fh.SIDE_USER), one.get_embeddings(fh.SIDE_ITEM),
                    one.pp_predictions(fh.SIDE_USER, p.nnz))
            for x in ranks:
                lo, hi = x.shard_range(side)
                assert 0 < hi - lo < x.n[side]  # the refresh has rows to replay
                np.testing.assert_array_equal(x.get_embeddings(fh.SIDE_USER), want[0])
                np.testing.assert_array_equal(x.get_embeddings(fh.SIDE_ITEM), want[1])
                np.testing.assert_array_equal(x.pp_predictions(fh.SIDE_USER, p.nnz), want[2])
        assert (want[0][:, s:e] != c.U[:, s:e]).any() and (want[1][:, s:e] != c.V[:, s:e]).any()
    finally:
        for x in ctxs:
            x.close()


def test_not_spd_reported_by_every_tile_count(monkeypatch):
    """A negative lambda (reg = -50, as test_parity_gpu.test_not_spd_reported
    for the full solve) makes every live entity's block matrix indefinite:
    pp_step of each TB reports FRECSYS_ERR_NOT_SPD with the smallest failing
    entity, and the next valid step on the same context is clean again."""
    ctx, p = _context(monkeypatch, "ials_user", 256)
    c = p.c
    for tb, bs in enumerate((8, 40, 70, 128), start=1):
        assert P.tile_count(bs) == tb
        assert (P.min_eigenvalues(p, 0, bs, -50.0) < 0).all()
        _reset(ctx, c)
        with pytest.raises(fh.FrecsysError) as ei:
            _step(ctx, c, 0, bs, reg=-50.0)
        assert ei.value.code == fh.ERR_NOT_SPD
        assert ei.value.entity == int(p.live[0]) == 1
    # the fail word was cleared: a fresh start and a valid step meet the bar
    s, e = 0, 128
    assert (s, e) in P.BLOCKS[256]
    _reset(ctx, c)
    resid = _step(ctx, c, s, e)
    E, other, pred = _read(ctx, c, p)
    ref, = P.reference("ials_user", 256, (s, e))
    _against_float64(p, ref, E, pred, resid, "after NOT_SPD")
    _untouched_outside(c, s, e, E, other)
