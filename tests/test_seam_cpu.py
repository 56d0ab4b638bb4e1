"""The seam fixture's contract (tests/seam_data.py), checked without a GPU:
the properties under which test_seam_gpu.py means anything, and the fp32 C
oracle alone against the float64 reference on it -- at most a quarter of the
project's 1e-4 row bar, so a GPU row that misses the bar against float64 is
the kernel's doing, not the restatement's.
"""
import numpy as np
import pytest

import seam_data as S
from conftest import rel_rows

ORACLE_CAP = 2.5e-5  # a quarter of TOL_ROW = 1e-4


@pytest.fixture(scope="module", params=["user", "item"])
def oriented(request):
    """(solved side's ptr, col, labels, other side's ptr, col) for the seam
    entities as users and as items."""
    sd = S.seam_data()
    if request.param == "user":
        nu, ni, up, uc, ip, ic = S.as_users(sd)
        return up, uc, sd.labels, ip, ic
    nu, ni, up, uc, ip, ic = S.as_items(sd)
    return ip, ic, sd.labels, up, uc


def test_histories_survive_the_csr(oriented):
    """Both CSRs come from one file-order pair list: the solved side's rows
    are the histories as drawn (order and repeats kept), the other side's
    are their transpose."""
    ptr, col, labels, optr, ocol = oriented
    sd = S.seam_data()
    assert len(ptr) - 1 == len(sd.hists) and len(optr) - 1 == S.N_OTHER
    for e, hist in enumerate(sd.hists):
        np.testing.assert_array_equal(col[ptr[e]:ptr[e + 1]], hist)
    assert col.min() == 0 and col.max() == S.N_OTHER - 1
    counts = np.bincount(col, minlength=S.N_OTHER)
    np.testing.assert_array_equal(np.diff(optr), counts)
    for r in (0, 1, S.N_OTHER - 1):
        mine = [e for e, hist in enumerate(sd.hists) for _ in range(int((hist == r).sum()))]
        np.testing.assert_array_equal(ocol[optr[r]:optr[r + 1]], mine)


def test_every_listed_length_present(oriented):
    ptr, col, labels, _, _ = oriented
    h = np.diff(ptr)
    want = [1, 2] + [32 * t + k for t in range(1, 17) for k in (-1, 0, 1)] + [639, 640]
    assert sorted(S.EDGE_LENGTHS) == want
    for x in want:
        assert (h == x).any(), x
    # under the tail quirk: the lengths that move, and where they land
    he = S.h_eff(h, True)
    for x, to in S.QUIRK_HEFF.items():
        assert x + 128 - x % 128 == to
        assert (he[h == x] == to).all() and (h == x).any(), (x, to)
    for x in (128, 256, 384, 512, 640):  # full blocks stay
        assert (he[h == x] == x).all()
    np.testing.assert_array_equal(he[h <= 128], h[h <= 128])
    # above 128 the quirk leaves whole blocks only: each one reached from
    # below (h % 128 != 0) and by a full history
    assert set(he[h > 128].tolist()) == {256, 384, 512, 640}
    for x in (256, 384, 512, 640):
        assert ((he == x) & (h < x)).any() and ((he == x) & (h == x)).any(), x
    # plain h is what every kind but ProjectV-with-quirk sees
    np.testing.assert_array_equal(S.h_eff(h, False), h)


def test_repeats_extremes_idle_and_zero_weights(oriented):
    ptr, col, labels, optr, ocol = oriented
    h = np.diff(ptr)
    hists = [col[ptr[e]:ptr[e + 1]] for e in range(len(h))]
    n = S.N_OTHER
    rep = [e for e, x in enumerate(hists) if len(x) and len(np.unique(x)) < len(x)]
    assert len(rep) >= 3
    assert sorted(h[rep]) == [33, 64, 257]
    for e in rep:  # moderate: no history is one row over and over
        assert len(np.unique(hists[e])) >= 20
    assert any(len(x) <= 2 and 0 in x for x in hists if len(x))
    assert any(len(x) <= 2 and n - 1 in x for x in hists if len(x))
    assert any(len(x) == 2 and 0 in x and n - 1 in x for x in hists)
    assert any(len(x) == 32 and x.min() == n - 32 for x in hists)
    assert any(len(x) == 33 and x.min() == n - 33 for x in hists)
    idle = np.nonzero(h == 0)[0]
    assert idle[0] == 0 and idle[-1] == len(h) - 1 and len(idle) >= 3
    assert ((idle > 0) & (idle < len(h) - 1)).any()
    assert labels.count("filler") == 40
    fill = h[[e for e, l in enumerate(labels) if l == "filler"]]
    assert fill.min() >= 3 and fill.max() < 200
    # V kinds: nu = 0 on every 9th row of the other side, never the first or the last
    c = S.seam_case("weighted_v_quirk", 8)
    zero_nu = c.other_weight == 0
    np.testing.assert_array_equal(np.nonzero(zero_nu)[0], np.arange(S.NU_ZERO[0], n, S.NU_ZERO[1]))
    assert not zero_nu[0] and not zero_nu[n - 1]
    all_zero = [e for e, x in enumerate(c.col[c.ptr[e]:c.ptr[e + 1]] for e in range(len(c.h)))
                if len(x) and zero_nu[x].all()]
    assert all_zero and all(c.labels[e] == "nu0" for e in all_zero)
    assert (c.entity_reg[c.h > 0] > 0).all()
    # U kinds: omega = 0 on every 11th seam entity, in the wave kernel's range,
    # the tridiagonal buckets, the wide bucket and d space
    cu = S.seam_case("weighted_u", 8)
    z = np.nonzero(cu.entity_weight == 0)[0]
    np.testing.assert_array_equal(z, np.arange(S.OMEGA_ZERO[0], len(cu.h), S.OMEGA_ZERO[1]))
    assert {63, 161, 288, 415, 513} <= set(cu.h[z].tolist())


KIND_KEYS = ["ials_user", "ials_item", "ials_exp0", "weighted_u", "weighted_v_quirk",
             "weighted_v_plain"]


@pytest.mark.parametrize("dim", [64, 100, 256])
@pytest.mark.parametrize("key", KIND_KEYS)
def test_oracle_within_a_quarter_of_the_bar(key, dim):
    """Measured on this fixture (max row error of the oracle against float64
    over the six kinds): 1.4e-6 at d = 64, 1.7e-6 at d = 100, 2.9e-6 at
    d = 256 (and 3.3e-6 at d = 500, 5.7e-6 at d = 1000, which
    test_seam_gpu.py asserts where it runs them)."""
    c = S.seam_case(key, dim)
    ref = S.reference(c)
    out = S.oracle_step(c)
    live = c.h > 0
    err = rel_rows(out[live], ref[live])
    worst = np.nonzero(live)[0][int(err.argmax())]
    print(f"seam oracle vs float64: {key} d={dim} max {err.max():.2e} "
          f"(h = {c.h[worst]}, {c.labels[worst]})")
    assert err.max() < ORACLE_CAP, (err.max(), int(c.h[worst]), c.labels[worst])
    np.testing.assert_array_equal(out[~live], c.E[~live])
    np.testing.assert_array_equal(ref[~live], c.E[~live].astype(np.float64))
    if c.kind == 1:
        zero = live & (c.entity_weight == 0)
        assert zero.sum() >= 5 and np.abs(ref[zero]).max() == 0.0 and np.abs(out[zero]).max() == 0.0
    if c.kind == 2:
        zero = np.array([l == "nu0" for l in c.labels])
        assert np.abs(ref[zero]).max() == 0.0 and np.abs(out[zero]).max() == 0.0


@pytest.mark.parametrize("key", ["cvar_u", "cvar_v"])
def test_oracle_cvar_steps(key):
    c = S.seam_case(key, 64)
    ref = S.reference(c)
    out = S.oracle_step(c)
    live = c.h > 0
    err = rel_rows(out[live], ref[live])
    print(f"seam oracle vs float64: {key} d=64 max {err.max():.2e}")
    assert err.max() < ORACLE_CAP
