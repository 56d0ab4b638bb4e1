"""The aux fixture's contract (tests/aux_data.py), checked without a GPU: the
conditions under which test_aux_gpu.py and the top-K cases of
test_topk_gpu.py mean anything.

* the fixture is what its docstring says;
* the fp32 C oracle alone stays within a quarter of the Gramian and loss bars
  against float64, so a GPU value past a bar is the kernel's doing (where it
  does not, aux_data.GRAM_ORACLE_ERR lists its error and the bar is 4 x that);
* one wrong gathered row in a long history moves the float64 loss by more
  than ten times the loss bar (the 0.1 init fails this);
* at most 5 % of the rows of a top-K case have two listed scores that fp32
  cannot be asked to tell apart.
"""
import itertools

import numpy as np
import pytest

import aux_data as A
import numpy_ref as R
import oracle as O

LOSS_TOL = 2e-5
LOSS_DIMS = (8, 16, 20, 64, 96, 128, 160, 224, 256, 500, 1000)


def test_fixture_contract():
    nu, ni, up, uc, ip, ic = A.aux_users()
    assert nu == A.N_USERS == 121 and ni == 704
    assert nu % 4 == 1 and nu > 64 and nu % 64 != 0
    h = np.diff(up)
    assert tuple(np.nonzero(h == 0)[0]) == A.IDLE == (0, 61, 114, 120)
    want = [1, 2] + [32 * t + k for t in range(1, 17) for k in (-1, 0, 1)] + [639, 640]
    for x in want + list(range(3, 19)):
        assert (h == x).any(), x
    assert uc.min() == 0 and uc.max() == ni - 1
    np.testing.assert_array_equal(np.diff(ip), np.bincount(uc, minlength=ni))
    # deterministic
    A._cache.pop("users")
    again = A.aux_users()
    for a, b in zip((up, uc, ip, ic), again[2:]):
        np.testing.assert_array_equal(a, b)
    # the loss's EVAL slice: 70 rows, more than one quad tile, row 0 not empty,
    # and an idle TRAIN user (0, 61) below 70 whose EVAL row has a history
    ep, ec = A.eval_slice(up, uc)
    assert len(ep) - 1 == 70 and ep[1] > ep[0]
    assert ep[1] - ep[0] > 0 and ep[62] - ep[61] > 0


def test_scaled_embeddings_scale():
    for dim in (8, 64, 1000):
        U, V = A.scaled_embeddings(dim, 121, 704, 3)
        assert U.dtype == V.dtype == np.float32 and U.shape == (121, dim) and V.shape == (704, dim)
        p = U.astype(np.float64) @ V.astype(np.float64).T
        assert 0.45 < p.std() < 0.55, p.std()
        U2, _ = A.scaled_embeddings(dim, 121, 704, 3)
        np.testing.assert_array_equal(U, U2)


def test_aux_eval_rows():
    for m, k in ((1025, 1024), (129, 129), (257, 33), (1, 1)):
        ep, ec = A.aux_eval(65, m, k, 5)
        h = np.diff(ep)
        assert h[0] == 0
        assert ec.min() >= 0 and ec.max() < m
        assert set(ec[ep[1]:ep[2]].tolist()) == {0, m - 1}
        r2 = ec[ep[2]:ep[3]]
        assert len(set(r2.tolist())) < len(r2)
        r3 = ec[ep[3]:ep[4]]
        assert len(r3) == len(set(r3.tolist())) == m - k + 1
        assert h[4:].min() >= 1 and h[4:].max() <= 40
    ep, ec = A.aux_eval(1, 128, 1, 5)
    assert len(ep) == 2 and ep[1] == 0


@pytest.mark.parametrize("dim,n", A.gram_cases())
def test_oracle_gramian_share(dim, n):
    X, w = A.gram_rows(dim, n)
    assert (w[3::7] == 0).all() and (np.delete(w, np.s_[3::7]) > 0).all()
    bar, worst = A.gram_bar(dim, n), 0.0
    for weights in (None, w):
        e = A.gram_err(O.gramian(X, weights), R.gram64(X, weights))
        worst = max(worst, e)
        print(f"oracle gramian d={dim} n={n} {'w' if weights is not None else 'plain'}: {e:.2e} "
              f"(bar {bar:.1e})")
        assert e <= 0.25 * bar, (e, bar)
    # a case is listed with a bar of its own only where the oracle needs it
    assert ((dim, n) in A.GRAM_ORACLE_ERR) == (worst > 0.25 * A.GRAM_TOL)


def _loss_refs(dim):
    nu, ni, up, uc, ip, ic = A.aux_users()
    U, V = A.scaled_embeddings(dim, nu, ni, dim)
    return up, uc, U, V, R.gram64(V)


@pytest.mark.parametrize("dim", LOSS_DIMS)
def test_oracle_loss_share(dim):
    up, uc, U, V, G64 = _loss_refs(dim)
    live = np.diff(up) > 0
    for beta, half in itertools.product((0.0, 0.005), (False, True)):
        ref = R.user_loss_side(up, uc, U, V, G64, beta, half)
        lo = O.user_loss(up, uc, U, V, O.gramian(V), beta, half)
        e = float(np.max(np.abs(lo[live] - ref[live]) / np.abs(ref[live])))
        print(f"oracle loss d={dim} beta={beta} half={half}: {e:.2e}")
        assert e <= 0.25 * LOSS_TOL, e
        assert (ref[~live] == 0).all()


def _sensitivity(up, uc, U, V):
    """Median relative change of the float64 loss (beta = 0) over the users
    with h >= 256 when the last history id becomes (id + 1) % n_items."""
    h = np.diff(up)
    G0 = np.zeros((U.shape[1],) * 2)
    out = []
    for e in np.nonzero(h >= 256)[0]:
        hist = np.array(uc[up[e]:up[e + 1]])
        a = R.user_loss(hist, U[e], V, G0, 0.0, False)
        hist[-1] = (hist[-1] + 1) % V.shape[0]
        b = R.user_loss(hist, U[e], V, G0, 0.0, False)
        out.append(abs(b - a) / a)
    assert len(out) >= 20
    return float(np.median(out))


@pytest.mark.parametrize("dim", LOSS_DIMS)
def test_loss_sees_one_wrong_row(dim):
    nu, ni, up, uc, ip, ic = A.aux_users()
    U, V = A.scaled_embeddings(dim, nu, ni, dim)
    s = _sensitivity(up, uc, U, V)
    U0, V0 = O.init_embeddings(1, 0.1, dim, nu, ni)
    s0 = _sensitivity(up, uc, U0, V0)
    print(f"loss sensitivity d={dim}: scaled {s:.2e}, 0.1 init {s0:.2e} (needs > {10 * LOSS_TOL:.0e})")
    assert s > 10 * LOSS_TOL
    assert s0 < 10 * LOSS_TOL  # why the loss tests do not use the 0.1 init


def test_topk_cases_cover_pairs():
    plan = A.topk_plan()
    vals = [A.TOPK_M, A.TOPK_ROWS, A.TOPK_KINDS, A.TOPK_DIMS]
    for a, b in itertools.combinations(range(4), 2):
        seen = {(c[a], c[b]) for c in plan}
        for pair in itertools.product(vals[a], vals[b]):
            assert pair in seen, (a, b, pair)
    mk = {(m, k) for m, _, k, _, _ in A.topk_cases()}
    assert {(1, 1), (129, 129), (1024, 1024), (1025, 1024)} <= mk
    assert {(m, 33) for m in A.TOPK_M if m >= 33} <= mk
    assert {(m, 1) for m in A.TOPK_M} <= mk


@pytest.mark.parametrize("m,rows,k,dim,seed", A.topk_cases())
def test_topk_gap_condition(m, rows, k, dim, seed):
    Ue, V, ep, ec, S, ref, close = A.topk_inputs(m, rows, k, dim, seed)
    print(f"topk m={m} rows={rows} k={k} d={dim}: {int(close.sum())} close rows")
    assert close.sum() <= 0.05 * rows
    if rows > 3:
        assert not close[3]
        # row 3: k - 1 free items, then the lowest excluded id
        free = np.isfinite(S[3])
        assert free.sum() == k - 1
        assert ref[3, -1] == np.nonzero(~free)[0][0]
        assert free[ref[3, :-1]].all()
