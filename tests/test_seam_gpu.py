"""Every history-length seam of the solve paths against float64.

The fixture (tests/seam_data.py) has an entity on each side of every
partition point, bucket bound, slab edge and tail-quirk landing, plus
repeated ids, the first / last row of the other side in one- and two-row
histories, idle entities at both ends and zero weights.  Each case is one
half-step through the C-ABI, compared with the float64 restatement of
tests/numpy_ref.py -- not with the fp32 oracle, whose own error on this
fixture test_seam_cpu.py caps at a quarter of the bar.

Modes (every FRECSYS_* variable of the environment is dropped first):
  default       no override at all: the shipped dispatch
  dspace        FRECSYS_DUAL=0
  dspace_split  FRECSYS_DUAL=0 FRECSYS_SPLIT_ROWS=64 at 32 <= Dp <= 256: slab
                edges at 128 | 129, 192 | 193, 256 | 257
  hspace_max    FRECSYS_DUAL_MAX_H=256 at 64 <= Dp <= 256 (the TH = 8 bucket),
                512 at Dp = 512 (the wide bucket up to 512 rows); at Dp = 1024
                that is the default
Worst row, its history length and the oracle's own float64 error go to
parity_report.jsonl (test = "seams").
"""
import os
import types

import numpy as np
import pytest

import seam_data as S
from conftest import rel_rows
from test_models_gpu import report

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

TOL_ROW = 1e-4

PADDED = {8: 8, 20: 32, 64: 64, 100: 128, 200: 224, 256: 256, 500: 512, 1000: 1024}  # dim: Dp
DIMS = list(PADDED)
SOLVE_KEYS = ["ials_user", "ials_item", "ials_exp0", "weighted_u", "weighted_v_quirk",
              "weighted_v_plain"]
MODES = ["default", "dspace", "dspace_split", "hspace_max"]

_runs = {}


def _mode_env(mode, Dp):
    """The overrides of a mode at this padded dim; None where the mode does
    not apply (no such case is generated)."""
    if mode == "default":
        return {}
    if mode == "dspace":
        return {"FRECSYS_DUAL": "0"}
    if mode == "dspace_split":
        return {"FRECSYS_DUAL": "0", "FRECSYS_SPLIT_ROWS": "64"} if 32 <= Dp <= 256 else None
    if mode == "hspace_max":
        if 64 <= Dp <= 256:
            return {"FRECSYS_DUAL_MAX_H": "256"}
        return {"FRECSYS_DUAL_MAX_H": "512"} if Dp == 512 else None
    raise ValueError(mode)


def _gpu_run(monkeypatch, key, dim, mode):
    """One half-step of case (key, dim) under `mode`, run once per session."""
    if (key, dim, mode) in _runs:
        return _runs[key, dim, mode]
    env = _mode_env(mode, fh.padded_dim(dim))
    for k in [k for k in os.environ if k.startswith("FRECSYS_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = S.seam_case(key, dim)
    ctx = fh.Context(dim, c.nu, c.ni, parity_quirks=c.quirk)
    ctx.load_csr(fh.SIDE_USER, c.up, c.uc)
    ctx.load_csr(fh.SIDE_ITEM, c.ip, c.ic)
    ctx.set_embeddings(fh.SIDE_USER, c.U)
    ctx.set_embeddings(fh.SIDE_ITEM, c.V)
    side, other = (fh.SIDE_USER, fh.SIDE_ITEM) if c.seam == "user" else (fh.SIDE_ITEM, fh.SIDE_USER)
    ctx.gramian(other, weights=c.gram_weights, fetch=False)
    kw = {}
    if c.kind == fh.KIND_IALS:
        kw = dict(reg_exp=c.reg_exp)
    elif c.kind in (fh.KIND_WEIGHTED_U, fh.KIND_CVAR_GRAD_U):
        kw = dict(entity_weight=c.entity_weight)
    else:
        kw = dict(alpha=c.alpha, entity_reg=c.entity_reg, other_weight=c.other_weight)
    if c.kind in (fh.KIND_CVAR_GRAD_U, fh.KIND_CVAR_GRAD_V):
        kw["stepsize"] = c.eta
    ctx.solve_side(side, c.kind, c.reg, c.w, **kw)
    tag = "solve_user" if c.seam == "user" else "solve_item"
    r = types.SimpleNamespace(out=ctx.get_embeddings(side), n_hs=ctx.work(tag + ".hspace")[2],
                              n_split=ctx.work(tag + ".split")[2],
                              reruns=ctx.counter("hspace_reruns"),
                              max_h=ctx.history_space_max_h(side), env=env)
    ctx.close()
    r.out.setflags(write=False)
    _runs[key, dim, mode] = r
    return r


def _rows_against_float64(c, out, what):
    """Every non-empty row at the bar, the offenders named by history length."""
    ref = S.reference(c)
    live = np.nonzero(c.h > 0)[0]
    err = rel_rows(out[live], ref[live])
    bad = [(int(c.h[e]), c.labels[e], float(x)) for e, x in zip(live, err) if not x < TOL_ROW]
    worst = live[int(np.argmax(err))]
    print(f"seams {what}: worst row {err.max():.2e} at h = {c.h[worst]} ({c.labels[worst]})")
    return err, worst, bad


def _check(monkeypatch, key, dim, mode):
    Dp = fh.padded_dim(dim)
    assert Dp == PADDED[dim]
    c = S.seam_case(key, dim)
    r = _gpu_run(monkeypatch, key, dim, mode)
    out = r.out
    err, worst, bad = _rows_against_float64(c, out, f"{key} d={dim} {mode}")
    orc = S.oracle_step(c)
    live = c.h > 0
    e_or = rel_rows(orc[live], S.reference(c)[live])
    report(test="seams", kind=key, dim=dim, mode=mode, env=r.env, max_row=float(err.max()),
           worst_h=int(c.h[worst]), worst_h_eff=int(c.h_eff[worst]), worst_label=c.labels[worst],
           f64_oracle_same_row=float(e_or[int(np.argmax(err))]), f64_oracle_max=float(e_or.max()),
           hspace_entities=r.n_hs, margin=TOL_ROW / max(float(err.max()), 1e-30))
    assert e_or.max() < 0.25 * TOL_ROW  # the restatement's own share of the bar
    assert not bad, f"rows (h, label, error) past {TOL_ROW}: {bad}"
    assert err.max() < TOL_ROW
    # idle rows untouched; zero-weight rows exactly zero
    np.testing.assert_array_equal(out[~live], c.E[~live])
    assert (~live).sum() >= 3
    if c.kind == fh.KIND_WEIGHTED_U:
        zero = live & (c.entity_weight == 0)
        assert zero.sum() >= 5
        assert np.abs(out[zero]).max() == 0.0, c.h[zero][np.abs(out[zero]).max(1) > 0]
    if c.kind == fh.KIND_WEIGHTED_V:
        zero = np.array([l == "nu0" for l in c.labels])
        assert zero.sum() == 1 and np.abs(out[zero]).max() == 0.0
    # the partition point: an entity exactly at the threshold is in history
    # space, one past it is not
    assert r.reruns == 0
    grad = c.kind in (fh.KIND_CVAR_GRAD_U, fh.KIND_CVAR_GRAD_V)
    off = Dp < 64 or grad or r.env.get("FRECSYS_DUAL") == "0"
    want = 0 if off else int(((c.h_eff > 0) & (c.h_eff <= r.max_h)).sum())
    assert r.n_hs == want, (r.n_hs, want, r.max_h)
    if mode == "default" and 64 <= Dp <= 256 and not grad:
        # the long ones run the same d-space kernel either way
        assert r.max_h == 224
        d = _gpu_run(monkeypatch, key, dim, "dspace")
        long = c.h_eff > r.max_h
        assert long.sum() >= 10
        np.testing.assert_array_equal(out[long], d.out[long])
    if mode == "dspace_split":
        # slabs of 64 rows for every entity with more than 128 assembly rows:
        # 129 is the first (its last slab is one row), 128 is not
        assert r.n_split == int((c.h_eff > 128).sum()) > 0
    else:
        assert r.n_split == 0  # the default slabs are 4,096 rows
    if mode == "hspace_max":
        assert r.max_h == (256 if Dp <= 256 else 512)


@pytest.mark.parametrize("key,dim,mode", [(k, d, m) for m in MODES for d in DIMS for k in SOLVE_KEYS
                                          if _mode_env(m, PADDED[d]) is not None])
def test_seam_rows_vs_float64(monkeypatch, key, dim, mode):
    _check(monkeypatch, key, dim, mode)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("key", ["cvar_u", "cvar_v"])
def test_seam_cvar_steps_vs_float64(monkeypatch, key, dim):
    _check(monkeypatch, key, dim, "default")
