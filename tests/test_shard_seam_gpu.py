"""The sharded solve, Gramian, loss and block step at their shard seams.

Ranks are W contexts of one process on device 0 in external-exchange mode
(tests/shard_data.py); every rank is checked on its own, before any row
exchange, so a rank that wrote a neighbour's row is seen:

  solve     seam and skew fixtures, all eight kinds, the Gramian through the
            group exchange: the rows of the shard within 1e-4 of float64 and
            bitwise the world-1 rows, every other row and every idle row with
            the start bits, omega = 0 / nu = 0 rows exactly 0, the history-
            space and split entity counts those of the shard, no rerun; an
            empty or idle-only shard leaves the table alone, twice.
  subsets   rank 0 of 8 through a change of its rotation row list on one
            context (plain pass -> subset -> plain, subset -> another subset,
            the latter also with the Gramian formed again in between):
            bitwise a fresh context's result each time.
  cg        skew fixture: bitwise world 1, -1 iterations outside the shard,
            counters untouched on ranks without work.
  loss      skew fixture as users: 2e-5 of float64, bitwise world 1, 0 for
            idle rows and for the other ranks' rows (frecsys_hip.h), also
            after an EVAL loss on the same context.
  gramian   row counts that give fewer groups than ranks: ranks that own
            nothing, slabs outside the own groups zero, G bitwise world 1
            on every rank and at the bar of test_aux_gpu.py.
  pp        skew fixture, W = 4: [0, 65), [65, 193), [193, 200) at d = 200 --
            the 135 columns behind [0, 65) in two steps, since a block holds
            at most 128 -- with pp_sync; bitwise the single rank, 1e-4 of
            float64.
One line per case goes to parity_report.jsonl (test = "shard_seams").
"""
import os
import types

import numpy as np
import pytest

import aux_data as A
import numpy_ref as R
import pp_ref as P
import seam_data as S
import shard_data as D
from conftest import rel_rows
from test_models_gpu import report

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

TOL_ROW = 1e-4
LOSS_TOL = 2e-5  # test_aux_gpu.py
DIMS = (8, 64, 256, 500, 1000)
SPLIT_ENV = {"FRECSYS_DUAL": "0", "FRECSYS_SPLIT_ROWS": "64"}

_single = {}


def _env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith("FRECSYS_")]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _sides(c):
    return (fh.SIDE_USER, fh.SIDE_ITEM) if c.seam == "user" else (fh.SIDE_ITEM, fh.SIDE_USER)


def _tag(c):
    return "solve_user" if c.seam == "user" else "solve_item"


def _make(c, world=1, rank=0):
    ctx = fh.Context(c.dim, c.nu, c.ni, device=0, parity_quirks=c.quirk)
    if world > 1:
        ctx.comm_init(world, rank, None)
    ctx.load_csr(fh.SIDE_USER, c.up, c.uc)
    ctx.load_csr(fh.SIDE_ITEM, c.ip, c.ic)
    ctx.set_embeddings(fh.SIDE_USER, c.U)
    ctx.set_embeddings(fh.SIDE_ITEM, c.V)
    return ctx


def _close(ctxs):
    for x in ctxs:
        x.close()


def _solve_kw(c):
    if c.kind == fh.KIND_IALS:
        kw = dict(reg_exp=c.reg_exp)
    elif c.kind in (fh.KIND_WEIGHTED_U, fh.KIND_CVAR_GRAD_U):
        kw = dict(entity_weight=c.entity_weight)
    else:
        kw = dict(alpha=c.alpha, entity_reg=c.entity_reg, other_weight=c.other_weight)
    if c.kind in (fh.KIND_CVAR_GRAD_U, fh.KIND_CVAR_GRAD_V):
        kw["stepsize"] = c.eta
    return kw


def _counts(ctx, c):
    return ctx.work(_tag(c) + ".hspace")[2], ctx.work(_tag(c) + ".split")[2]


def _assembly_rows(c):
    """h_eff as ctx.h queue_heff counts it: the tail quirk for both V kinds."""
    return S.h_eff(c.h, c.quirk and c.kind in (fh.KIND_WEIGHTED_V, fh.KIND_CVAR_GRAD_V))


def _single_solve(fixture, key, dim, mode):
    """World 1, one context per (fixture, kind, d, mode), run once."""
    k = (fixture, key, dim, mode)
    if k not in _single:
        c = D.case(fixture, key, dim)
        side, other = _sides(c)
        with _make(c) as ctx:
            G = ctx.gramian(other, weights=c.gram_weights)
            ctx.solve_side(side, c.kind, c.reg, c.w, **_solve_kw(c))
            n_hs, n_split = _counts(ctx, c)
            r = types.SimpleNamespace(out=ctx.get_embeddings(side), G=G, n_hs=n_hs, n_split=n_split,
                                      max_h=ctx.history_space_max_h(side),
                                      reruns=ctx.counter("hspace_reruns"),
                                      timeouts=ctx.counter("tagged_timeouts"))
        r.out.setflags(write=False)
        _single[k] = r
    return _single[k]


def _check_sharded_solve(monkeypatch, fixture, key, dim, world, mode):
    env = SPLIT_ENV if mode == "split" else {}
    _env(monkeypatch, env)
    c = D.case(fixture, key, dim)
    Dp = fh.padded_dim(dim)
    side, other = _sides(c)
    one = _single_solve(fixture, key, dim, mode)
    assert (one.reruns, one.timeouts) == (0, 0), "world 1 fell back to the d-space solve"
    ref = S.reference(c)
    bounds = D.BOUNDS[fixture, world]
    n = len(c.h)
    live = c.h > 0
    he = _assembly_rows(c)
    grad = c.kind in (fh.KIND_CVAR_GRAD_U, fh.KIND_CVAR_GRAD_V)
    hs_off = Dp < 64 or grad or mode == "split"
    full = np.array(c.E)
    worst = (0.0, -1, -1)  # error, h, rank
    hs_ranks, split_ranks, no_work = [], [], []
    ctxs = [_make(c, world, r) for r in range(world)]
    try:
        G = D.allreduce_gram(ctxs, other, c.gram_weights)
        np.testing.assert_array_equal(G, one.G)
        for r, ctx in enumerate(ctxs):
            lo, hi = ctx.shard_range(side)
            assert (lo, hi) == (bounds[r], bounds[r + 1]), (r, lo, hi)
            mine = np.zeros(n, bool)
            mine[lo:hi] = True
            ctx.solve_side(side, c.kind, c.reg, c.w, **_solve_kw(c))  # raises unless FRECSYS_OK
            out = ctx.get_embeddings(side)
            # nothing outside the shard, no idle row
            np.testing.assert_array_equal(out[~mine], c.E[~mine], err_msg=f"rank {r} wrote outside")
            np.testing.assert_array_equal(out[~live], c.E[~live])
            assert ctx.counter("hspace_reruns") == 0, r
            diff = [(int(e), int(c.h[e])) for e in range(lo, hi) if (out[e] != one.out[e]).any()]
            assert not diff, f"rank {r}: rows (entity, h) not bitwise the world-1 rows: {diff}"
            sel = mine & live
            if sel.any():
                err = rel_rows(out[sel], ref[sel])
                idx = np.nonzero(sel)[0]
                bad = [(int(c.h[e]), c.labels[e], float(x)) for e, x in zip(idx, err)
                       if not x < TOL_ROW]
                assert not bad, f"rank {r}: rows (h, label, error) past {TOL_ROW}: {bad}"
                if err.max() >= worst[0]:
                    worst = (float(err.max()), int(c.h[idx[int(err.argmax())]]), r)
            if c.kind == fh.KIND_WEIGHTED_U:
                zero = sel & (c.entity_weight == 0)
                assert not out[zero].any()
            if c.kind == fh.KIND_WEIGHTED_V and fixture == "seam":
                zero = sel & np.array([l == "nu0" for l in c.labels])
                assert not out[zero].any()
            n_hs, n_split = _counts(ctx, c)
            max_h = ctx.history_space_max_h(side)
            assert max_h == one.max_h
            want_hs = 0 if hs_off else int((mine & (he > 0) & (he <= max_h)).sum())
            want_split = int((mine & (he > 128)).sum()) if mode == "split" else 0
            assert n_hs == want_hs, (r, n_hs, want_hs)
            assert n_split == want_split, (r, n_split, want_split)
            assert (ctx.counter("hspace_reruns"), ctx.counter("tagged_timeouts")) == (0, 0), r
            hs_ranks.append(n_hs)
            split_ranks.append(n_split)
            if not sel.any():
                # an empty or idle-only shard: nothing to do, and again nothing
                no_work.append(r)
                np.testing.assert_array_equal(out, c.E)
                assert (n_hs, n_split) == (0, 0)
                ctx.solve_side(side, c.kind, c.reg, c.w, **_solve_kw(c))
                np.testing.assert_array_equal(ctx.get_embeddings(side), c.E)
                assert _counts(ctx, c) == (0, 0)
            full[lo:hi] = out[lo:hi]
    finally:
        _close(ctxs)
    assert sum(hs_ranks) == one.n_hs and sum(split_ranks) == one.n_split and one.reruns == 0
    np.testing.assert_array_equal(full, one.out)
    err = rel_rows(full[live], ref[live])
    assert err.max() < TOL_ROW
    if c.kind == fh.KIND_WEIGHTED_V and fixture == "seam":
        assert not full[np.array([l == "nu0" for l in c.labels])].any()
    print(f"shard_seams solve {fixture} {key} d={dim} W={world} {mode}: worst row {worst[0]:.2e} "
          f"(h = {worst[1]}, rank {worst[2]}); hspace {hs_ranks} split {split_ranks}")
    report(test="shard_seams", entry="solve", fixture=fixture, kind=key, dim=dim, world=world,
           mode=mode, max_row=worst[0], worst_h=worst[1], worst_rank=worst[2],
           hspace_entities=hs_ranks, split_entities=split_ranks, idle_ranks=no_work,
           margin=TOL_ROW / max(worst[0], 1e-30))
    return hs_ranks, split_ranks, no_work


SEAM_CASES = ([(k, d, w, "default") for d in DIMS for w in (3, 8) for k in S.KINDS] +
              [(k, d, 16, "default") for d in (64, 500) for k in S.KINDS] +
              [(k, d, 8, "split") for d in (64, 256) for k in S.KINDS])


@pytest.mark.parametrize("key,dim,world,mode", SEAM_CASES)
def test_seam_fixture_sharded_solve(monkeypatch, key, dim, world, mode):
    hs, split, no_work = _check_sharded_solve(monkeypatch, "seam", key, dim, world, mode)
    assert not no_work
    c = S.seam_case(key, dim)
    dual = fh.padded_dim(dim) >= 64 and c.kind < fh.KIND_CVAR_GRAD_U and mode == "default"
    live = [int((c.h[lo:hi] > 0).sum()) for lo, hi in D.shards(D.BOUNDS["seam", world])]
    if dual and world == 8 and fh.padded_dim(dim) <= 256 and (c.h_eff == c.h).all():
        # the three branches of train.hip solve_side: shard 0 wholly in history
        # space, shards 1-4 wholly in d-space, shard 5 mixed
        assert hs[0] == live[0] == 22 and hs[1:5] == [0, 0, 0, 0] and 0 < hs[5] < live[5]
    if dual and world == 3 and fh.padded_dim(dim) <= 256:
        assert hs[1] == 0 and live[1] == 14  # h = 384..513: d-space alone
    if mode == "split":
        # shards 1-4: every entity split; the others: some (every shard of
        # this world holds an entity past 128 rows, so none is without)
        assert split[1:5] == live[1:5] and all(0 < x < n for x, n in zip(split[:1] + split[5:],
                                                                        live[:1] + live[5:]))


@pytest.mark.parametrize("key,dim,world", [(k, d, w) for d in DIMS for w in D.WORLDS["skew"]
                                           for k in S.KINDS])
def test_skew_fixture_sharded_solve(monkeypatch, key, dim, world):
    hs, split, no_work = _check_sharded_solve(monkeypatch, "skew", key, dim, world, "default")
    assert no_work == {2: [], 3: [2], 4: [1, 3], 8: [1, 2, 3, 5, 6, 7]}[world]


# ---------------------------------------------------------------- rotation row subsets
SHARD0 = (0, 23)  # rank 0 of 8 on the seam fixture
VARIANTS = {"seamB": (0, 400, 101), "seamC": (300, 704, 102)}  # rows drawn from, seed
SEQUENCES = {"plain_subset_plain": (("seam", "seamB", "seam"), False),
             "subset_subset": (("seamB", "seamC", "seamB"), False),
             "subset_subset_regram": (("seamB", "seamC", "seamB"), True)}
_fresh = {}


def _variant_case(name, key, dim):
    if name != "seam":
        lo, hi, seed = VARIANTS[name]
        D.register_variant(name, SHARD0[0], SHARD0[1], lo, hi, seed)
    return D.case(name, key, dim)


def _load(ctx, c, side):
    ctx.load_csr(fh.SIDE_USER, c.up, c.uc)
    ctx.load_csr(fh.SIDE_ITEM, c.ip, c.ic)
    ctx.set_embeddings(side, c.E)  # the solved side back to its start; the other table stays


def _fresh_rank0(name, key, dim, G):
    if (name, key, dim) not in _fresh:
        c = _variant_case(name, key, dim)
        side, other = _sides(c)
        with _make(c, 8, 0) as ctx:
            ctx.set_gramian(other, G)
            ctx.solve_side(side, c.kind, c.reg, c.w, **_solve_kw(c))
            _fresh[name, key, dim] = ctx.get_embeddings(side)
    return _fresh[name, key, dim]


@pytest.mark.parametrize("seq", list(SEQUENCES))
@pytest.mark.parametrize("key,dim", [(k, d) for k in ("ials_user", "weighted_v_quirk")
                                     for d in (64, 500)])
def test_row_subset_changes_on_one_context(monkeypatch, key, dim, seq):
    """No stale row list and no stale rotated copy: the other side's table
    and Gramian stay, the CSR changes under them."""
    _env(monkeypatch)
    names, regram = SEQUENCES[seq]
    a = _variant_case("seam", key, dim)
    side, other = _sides(a)
    lo, hi = SHARD0
    with _make(a) as one:  # the whole Gramian, as every rank holds it after the exchange
        G = one.gramian(other, weights=a.gram_weights)
        max_h = one.history_space_max_h(side)
    # which pass rank 0 takes with each CSR (hspace_rows' rule, restated)
    reads = {}
    for nm in set(names):
        c = _variant_case(nm, key, dim)
        assert D.partition(c.ptr, 8)[:2] == [lo, hi]
        np.testing.assert_array_equal(c.gram_weights, a.gram_weights)
        np.testing.assert_array_equal(c.X, a.X)
        n_hs, n_rows = D.subset_rows(c, lo, hi, max_h)
        assert n_hs >= 13
        rows = set()
        for e in range(lo, hi):
            if 0 < c.h_eff[e] <= max_h:
                rows.update(c.col[c.ptr[e]:c.ptr[e + 1]].tolist())
        reads[nm] = (D.takes_subset(n_rows), rows)
    for nm, (subset, _) in reads.items():  # the seam CSR: plain pass; the variants: a list
        assert subset == (nm != "seam"), nm
    if "seamC" in reads:
        assert reads["seamB"][1] - reads["seamC"][1] and reads["seamC"][1] - reads["seamB"][1]
    worst = 0.0
    with _make(_variant_case(names[0], key, dim), 8, 0) as ctx:
        ctx.gramian(other, weights=a.gram_weights, fetch=False)
        ctx.set_gramian(other, G)
        for step, nm in enumerate(names):
            c = _variant_case(nm, key, dim)
            if step:
                _load(ctx, c, side)
                if regram:  # a Gramian formed with the last list still in place
                    ctx.gramian(other, weights=a.gram_weights, fetch=False)
                    ctx.set_gramian(other, G)
            assert ctx.shard_range(side) == (lo, hi)
            ctx.solve_side(side, c.kind, c.reg, c.w, **_solve_kw(c))
            out = ctx.get_embeddings(side)
            np.testing.assert_array_equal(out, _fresh_rank0(nm, key, dim, G),
                                          err_msg=f"step {step} ({nm}) vs a fresh context")
            np.testing.assert_array_equal(out[hi:], c.E[hi:])
            live = np.nonzero(c.h[lo:hi] > 0)[0]
            err = rel_rows(out[live], S.reference(c)[live])
            assert err.max() < TOL_ROW, (step, nm, float(err.max()), int(c.h[live[err.argmax()]]))
            worst = max(worst, float(err.max()))
            n_hs = D.subset_rows(c, lo, hi, max_h)[0]  # the same lengths, so the same count
            assert ctx.work(_tag(c) + ".hspace")[2] == (step + 1) * n_hs
            assert ctx.counter("hspace_reruns") == 0
    report(test="shard_seams", entry="row_subsets", kind=key, dim=dim, sequence=seq,
           subset=[bool(reads[nm][0]) for nm in names], max_row=worst,
           margin=TOL_ROW / max(worst, 1e-30))


# ---------------------------------------------------------------- conjugate gradients
_single_cg = {}


def _cg(ctx, c, side):
    kw = dict(alpha=getattr(c, "alpha", 0.0), reg_exp=getattr(c, "reg_exp", 1.0))
    if c.kind == fh.KIND_WEIGHTED_U:
        kw["entity_weight"] = c.entity_weight
    if c.kind == fh.KIND_WEIGHTED_V:
        kw.update(entity_reg=c.entity_reg, other_weight=c.other_weight)
    ctx.solve_side_cg(side, c.kind, c.reg, c.w, **kw)  # cg_ref's defaults: 100, 1e-10
    return ctx.get_embeddings(side), ctx.cg_iterations(side)


@pytest.mark.parametrize("world", [4, 8])
@pytest.mark.parametrize("dim", [8, 64, 256])
@pytest.mark.parametrize("key", ["ials_user", "weighted_u", "weighted_v_quirk"])
def test_skew_fixture_sharded_cg(monkeypatch, key, dim, world):
    _env(monkeypatch)
    c = D.case("skew", key, dim)
    side, other = _sides(c)
    if (key, dim) not in _single_cg:
        with _make(c) as ctx:
            ctx.gramian(other, weights=c.gram_weights, fetch=False)
            _single_cg[key, dim] = _cg(ctx, c, side)
    out1, it1 = _single_cg[key, dim]
    ref = S.reference(c)
    bounds = D.BOUNDS["skew", world]
    live = c.h > 0
    n = len(c.h)
    worst, idle_ranks = 0.0, []
    ctxs = [_make(c, world, r) for r in range(world)]
    try:
        D.allreduce_gram(ctxs, other, c.gram_weights)
        for r, ctx in enumerate(ctxs):
            lo, hi = ctx.shard_range(side)
            assert (lo, hi) == (bounds[r], bounds[r + 1])
            mine = np.zeros(n, bool)
            mine[lo:hi] = True
            before = (ctx.counter("cg_iterations"), ctx.counter("cg_unconverged"))
            out, it = _cg(ctx, c, side)
            np.testing.assert_array_equal(out[mine], out1[mine])
            np.testing.assert_array_equal(it[mine], it1[mine])
            np.testing.assert_array_equal(out[~mine], c.E[~mine])
            np.testing.assert_array_equal(out[~live], c.E[~live])
            assert (it[~mine] == -1).all() and (it[~live] == -1).all()
            sel = mine & live
            assert (it[sel] >= 0).all()
            conv = sel & (it < 100)
            if conv.any():
                err = rel_rows(out[conv], ref[conv])
                assert err.max() < TOL_ROW, (r, float(err.max()))
                worst = max(worst, float(err.max()))
            after = (ctx.counter("cg_iterations"), ctx.counter("cg_unconverged"))
            if not sel.any():
                idle_ranks.append(r)
                assert after == before
            else:
                assert after[0] - before[0] == int(it[sel].sum())
    finally:
        _close(ctxs)
    assert idle_ranks == {4: [1, 3], 8: [1, 2, 3, 5, 6, 7]}[world]
    assert (it1[live] < 100).all()  # every live row converged, so every live row was measured
    report(test="shard_seams", entry="cg", fixture="skew", kind=key, dim=dim, world=world,
           max_row=worst, margin=TOL_ROW / max(worst, 1e-30))


# ---------------------------------------------------------------- user loss
_loss = {}


def _loss_case(dim):
    if dim not in _loss:
        nu, ni, up, uc, ip, ic = D.fixture_data("skew")["user"]
        U, V = A.scaled_embeddings(dim, nu, ni, dim)
        c = types.SimpleNamespace(dim=dim, nu=nu, ni=ni, up=up, uc=uc, ip=ip, ic=ic, U=U, V=V,
                                  quirk=True, G64=R.gram64(V), single={}, ref={})
        _loss[dim] = c
    return _loss[dim]


@pytest.mark.parametrize("world", [4, 8])
@pytest.mark.parametrize("beta", [0.0, 0.005])
@pytest.mark.parametrize("dim", DIMS)
def test_skew_fixture_sharded_loss(monkeypatch, dim, beta, world):
    _env(monkeypatch)
    c = _loss_case(dim)
    half = beta > 0
    if beta not in c.single:
        with _make(c) as ctx:
            ctx.gramian(fh.SIDE_ITEM, fetch=False)
            c.single[beta] = ctx.user_loss(fh.SIDE_USER, beta, half)
        c.ref[beta] = R.user_loss_side(c.up, c.uc, c.U, c.V, c.G64, beta, half)
    one, ref = c.single[beta], c.ref[beta]
    h = np.asarray(D.SKEW_H)
    assert (ref[h == 0] == 0).all() and (ref[h > 0] != 0).all()
    bounds = D.BOUNDS["skew", world]
    worst = 0.0
    ctxs = [_make(c, world, r) for r in range(world)]
    try:
        D.allreduce_gram(ctxs, fh.SIDE_ITEM)
        for r, ctx in enumerate(ctxs):
            lo, hi = ctx.shard_range(fh.SIDE_USER)
            assert (lo, hi) == (bounds[r], bounds[r + 1])
            mine = np.zeros(len(h), bool)
            mine[lo:hi] = True
            got = ctx.user_loss(fh.SIDE_USER, beta, half)  # OK on the ranks without work too
            np.testing.assert_array_equal(got[mine], one[mine])
            assert (got[mine & (h == 0)] == 0).all()
            assert (got[~mine] == 0).all(), (r, got)  # frecsys_hip.h: the other ranks' rows read 0
            sel = mine & (h > 0)
            if sel.any():
                err = np.abs(got[sel] - ref[sel]) / np.abs(ref[sel])
                assert err.max() <= LOSS_TOL, (r, float(err.max()))
                worst = max(worst, float(err.max()))
            if r in (0, world - 1):
                # an EVAL loss in between must not show through in the other ranks' rows
                ctx.load_csr(fh.SIDE_EVAL, c.up, c.uc)
                ctx.set_embeddings(fh.SIDE_EVAL, c.U)
                ev = ctx.user_loss(fh.SIDE_EVAL, beta, half)
                assert (ev[h > 0] != 0).all()  # what would show through
                again = ctx.user_loss(fh.SIDE_USER, beta, half)
                np.testing.assert_array_equal(again, got)
    finally:
        _close(ctxs)
    report(test="shard_seams", entry="user_loss", fixture="skew", dim=dim, world=world, beta=beta,
           err=worst, bar=LOSS_TOL, margin=LOSS_TOL / max(worst, 1e-30))


# ---------------------------------------------------------------- Gramian
GRAM_CASES = ([(d, n) for d in (20, 64, 256) for n in (1, 33, 65, 1025, 1089)] +
              [(d, n) for d in (500, 1000) for n in (1, 17, 257, 4097)])
_gram = {}


def _gram_case(dim, n):
    if (dim, n) not in _gram:
        X, w = A.gram_rows(dim, n)
        with fh.Context(dim, n, 1, device=0) as ctx:
            ctx.set_embeddings(fh.SIDE_USER, X)
            one = [ctx.gramian(fh.SIDE_USER, weights=wt) for wt in (None, w)]
        _gram[dim, n] = (X, w, one, [R.gram64(X), R.gram64(X, w)])
    return _gram[dim, n]


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("dim,n", GRAM_CASES)
def test_gramian_on_ranks_without_groups(monkeypatch, dim, n, world):
    _env(monkeypatch)
    X, w, one, G64 = _gram_case(dim, n)
    bar = A.gram_bar(dim, n)
    ngroup = fh.gram_plan(dim, n)[2]
    ctxs = []
    try:
        for r in range(world):
            ctx = fh.Context(dim, n, 1, device=0)  # no CSR: the Gramian needs none
            ctx.comm_init(world, r, None)
            ctx.set_embeddings(fh.SIDE_USER, X)
            ctxs.append(ctx)
        for i, wt in enumerate((None, w)):
            D.allreduce_gram(ctxs, fh.SIDE_USER, wt)  # asserts the tiling and zero foreign slabs
            owned = [x.gram_groups(fh.SIDE_USER) for x in ctxs]
            assert all(o[0] == ngroup for o in owned)
            assert [o[1:3] for o in owned] == [fh.gram_plan(dim, n, world, r)[3:5]
                                               for r in range(world)]
            if ngroup < world:
                assert any(o[1] == o[2] for o in owned)
            for x in ctxs:
                np.testing.assert_array_equal(x.get_gramian(fh.SIDE_USER), one[i])
            e = A.gram_err(one[i], G64[i])
            assert e <= bar, (e, bar, i)
            report(test="shard_seams", entry="gramian", dim=dim, rows=n, world=world,
                   weighted=bool(i), groups=ngroup,
                   idle_ranks=int(sum(o[1] == o[2] for o in owned)), err=e, bar=bar,
                   margin=bar / max(e, 1e-30))
    finally:
        _close(ctxs)
    if n == 1:
        assert ngroup == 1  # fewer groups than ranks at every world used here


# ---------------------------------------------------------------- iALS++ block step
PP_BLOCKS = ((0, 65), (65, 193), (193, 200))


@pytest.mark.parametrize("key", ["ials_user", "weighted_v_plain"])
def test_skew_fixture_sharded_block_steps(monkeypatch, key):
    """W = 4 on the skew fixture (rank 1 empty, rank 3 idle-only), external
    exchange with pp_sync: iALS on the user side, ProjectV on the item side
    (the skew entities are the solved side in both)."""
    _env(monkeypatch)
    dim, world = 200, 4
    p = D.pp_case("skew", key, dim)
    c = p.c
    side, other = _sides(c)

    def make(w=1, r=0):
        ctx = _make(c, w, r)
        ctx.pp_set_rating_index(fh.SIDE_USER, p.urix)
        ctx.pp_set_rating_index(fh.SIDE_ITEM, p.irix)
        ctx.pp_predict(fh.SIDE_USER)
        return ctx

    def step(ctx, s, e):
        if c.kind == fh.KIND_IALS:
            return ctx.pp_step(side, s, e, c.reg, c.w, reg_exp=c.reg_exp)
        return ctx.pp_step(side, s, e, c.reg, c.w, kind=c.kind, alpha=c.alpha,
                           entity_reg=c.entity_reg, other_weight=c.other_weight)

    E64 = c.E.astype(np.float64)
    pred64 = P.predict(c.up, c.uc, p.urix, c.V, c.U)
    ctxs = [make()] + [make(world, r) for r in range(world)]
    worst_b = worst_p = 0.0
    try:
        one, ranks = ctxs[0], ctxs[1:]
        assert [x.shard_range(side) for x in ranks] == D.shards(D.BOUNDS["skew", world])
        one.gramian(other, weights=c.gram_weights, fetch=False)
        D.allreduce_gram(ranks, other, c.gram_weights)
        for s, e in PP_BLOCKS:
            r_one = step(one, s, e)
            r_sh = sum(step(x, s, e) for x in ranks)
            D.allgather_rows(ranks, side)
            for x in ranks:
                x.pp_sync(side)
            assert abs(r_sh - r_one) <= 1e-9 * r_one
            E1 = one.get_embeddings(side)
            pr1 = one.pp_predictions(fh.SIDE_USER, p.nnz)
            for x in ranks:
                np.testing.assert_array_equal(x.get_embeddings(side), E1)
                np.testing.assert_array_equal(x.get_embeddings(other), c.X)
                np.testing.assert_array_equal(x.pp_predictions(fh.SIDE_USER, p.nnz), pr1)
            E64, pred64, delta, dpred, res = P.block_step(c, p.rix, E64, pred64, s, e)
            ref = types.SimpleNamespace(s=s, e=e, E=E64, pred=pred64, delta=delta, dpred=dpred,
                                        residual=res)
            eb, ep = P.block_errors(p, ref, E1), P.pred_errors(p, ref, pr1)
            assert not P.offenders(p, eb, P.TOL), (s, e, P.offenders(p, eb, P.TOL))
            assert not P.offenders(p, ep, P.TOL), (s, e, P.offenders(p, ep, P.TOL))
            assert abs(r_one - res) <= 1e-4 * res
            worst_b, worst_p = max(worst_b, float(eb.max())), max(worst_p, float(ep.max()))
            np.testing.assert_array_equal(E1[c.h == 0], c.E[c.h == 0])
            assert (E1[p.live, s:e] != c.E[p.live, s:e]).any(axis=1).all()
    finally:
        _close(ctxs)
    report(test="shard_seams", entry="pp_step", fixture="skew", kind=key, dim=dim, world=world,
           max_block=worst_b, max_pred=worst_p, margin=P.TOL / max(worst_b, worst_p, 1e-30))
