"""The 64-bit gather-offset variants of the d-space kernels are bit-identical
to the 32-bit ones.

The split-bf16 SYRK gathers (solve_tiled_kernel, wide_syrk2_kernel) address
the other side's rows with 32-bit element offsets while n_other * Dp < 2^32
and dispatch 64-bit variants above that (kernels.h gather_off64: Dp = 256
beyond 16.7M rows, Dp = 1024 beyond 4.19M).  A table of that size takes
17 GB of host and device memory to build, so the dispatch is forced here with
FRECSYS_GATHER64=1 (read at every launch) and both widths must give the same
bits: every kind, the long-history split slabs included.

The history-space wave kernel (dual.hip dual_wave_kernel, h_eff <= 64) has the
same pair for the row offsets of its coalesced slab fetch, under the same
switch: test_wave_kernel_offsets_64_bit_identical runs it on the seam fixture
with the shipped dispatch (no FRECSYS_DUAL override).
"""
import os

import numpy as np
import pytest

import frecsys_hip as fh
import seam_data as S

pytestmark = pytest.mark.gpu


def _run(monkeypatch, quirk_data, dim, off64):
    nu, ni, up, uc, ip, ic = quirk_data
    monkeypatch.setenv("FRECSYS_GATHER64", "1" if off64 else "0")
    monkeypatch.setenv("FRECSYS_DUAL", "0")        # every entity on the d-space kernels
    monkeypatch.setenv("FRECSYS_SPLIT_ROWS", "64")  # long histories through the split slabs
    ctx = fh.Context(dim, nu, ni, device=0)
    ctx.load_csr(fh.SIDE_USER, up, uc)
    ctx.load_csr(fh.SIDE_ITEM, ip, ic)
    ctx.init_embeddings(1, 0.1)
    rng = np.random.default_rng(2)
    omega = rng.uniform(0.1, 1.0, nu).astype(np.float32)
    hu = np.diff(up).astype(np.float32)
    nu_w = np.where(hu > 0, omega / np.maximum(hu, 1), 0).astype(np.float32)
    item_reg = rng.uniform(0.5, 2.0, ni).astype(np.float32)
    out = []
    ctx.gramian(fh.SIDE_ITEM, fetch=False)
    ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, 0.003, 0.1)
    out.append(ctx.get_embeddings(fh.SIDE_USER))
    ctx.solve_side(fh.SIDE_USER, fh.KIND_WEIGHTED_U, 0.003, 0.1, entity_weight=omega)
    out.append(ctx.get_embeddings(fh.SIDE_USER))
    ctx.gramian(fh.SIDE_USER, weights=omega, fetch=False)
    out.append(ctx.get_gramian(fh.SIDE_USER))
    ctx.solve_side(fh.SIDE_ITEM, fh.KIND_WEIGHTED_V, 0.003, 0.1, alpha=0.3,
                   entity_reg=item_reg, other_weight=nu_w)
    out.append(ctx.get_embeddings(fh.SIDE_ITEM))
    ctx.snapshot(fh.SIDE_USER)
    ctx.solve_side(fh.SIDE_ITEM, fh.KIND_CVAR_GRAD_V, 0.003, 0.1, alpha=0.3, stepsize=0.01,
                   entity_reg=item_reg, other_weight=nu_w, from_snapshot=True)
    out.append(ctx.get_embeddings(fh.SIDE_ITEM))
    ctx.close()
    return out


@pytest.mark.parametrize("dim", [64, 256, 512, 1000])
def test_gather_offsets_64_bit_identical(monkeypatch, quirk_data, dim):
    a = _run(monkeypatch, quirk_data, dim, False)
    b = _run(monkeypatch, quirk_data, dim, True)
    for x, y in zip(a, b):
        assert np.all(np.isfinite(x))
        np.testing.assert_array_equal(x, y)


def _run_hspace(monkeypatch, key, dim, off64):
    for k in [k for k in os.environ if k.startswith("FRECSYS_")]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("FRECSYS_GATHER64", "1" if off64 else "0")
    c = S.seam_case(key, dim)
    ctx = fh.Context(dim, c.nu, c.ni, device=0, parity_quirks=c.quirk)
    ctx.load_csr(fh.SIDE_USER, c.up, c.uc)
    ctx.load_csr(fh.SIDE_ITEM, c.ip, c.ic)
    ctx.set_embeddings(fh.SIDE_USER, c.U)
    ctx.set_embeddings(fh.SIDE_ITEM, c.V)
    side, other = (fh.SIDE_USER, fh.SIDE_ITEM) if c.seam == "user" else (fh.SIDE_ITEM, fh.SIDE_USER)
    ctx.gramian(other, weights=c.gram_weights, fetch=False)
    if c.kind == fh.KIND_IALS:
        kw = dict(reg_exp=c.reg_exp)
    elif c.kind == fh.KIND_WEIGHTED_U:
        kw = dict(entity_weight=c.entity_weight)
    else:
        kw = dict(alpha=c.alpha, entity_reg=c.entity_reg, other_weight=c.other_weight)
    ctx.solve_side(side, c.kind, c.reg, c.w, **kw)
    tag = "solve_user" if c.seam == "user" else "solve_item"
    out = ctx.get_embeddings(side), ctx.work(tag + ".hspace")[2], ctx.counter("hspace_reruns")
    ctx.close()
    return out


@pytest.mark.parametrize("dim", [64, 256, 500, 1000])
@pytest.mark.parametrize("key", ["ials_user", "weighted_u", "weighted_v_quirk"])
def test_wave_kernel_offsets_64_bit_identical(monkeypatch, key, dim):
    a, n_a, reruns_a = _run_hspace(monkeypatch, key, dim, False)
    b, n_b, reruns_b = _run_hspace(monkeypatch, key, dim, True)
    c = S.seam_case(key, dim)
    assert ((c.h_eff > 0) & (c.h_eff <= 64)).sum() >= 10  # entities of the wave kernels
    assert n_a > 0 and n_b == n_a
    assert reruns_a == 0 and reruns_b == 0
    assert np.all(np.isfinite(a))
    np.testing.assert_array_equal(a, b)
