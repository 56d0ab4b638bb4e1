"""The host side of exact rank evaluation, no GPU: frecsys_position_metrics
against the Python-int / float64 reference of tests/positions_ref.py, its
argument errors, the reference ranks against recommend64's own lists, and the
cover of the GPU test's case plan.
"""
import itertools

import numpy as np
import pytest

import positions_ref as PR
import recommend_ref as RR

import frecsys_hip as fh


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(rank, gt_ptr, eligible):
    mrr, auc = fh.position_metrics(rank, gt_ptr, eligible)
    rm, ra = PR.position_metrics_ref(np.asarray(rank), np.asarray(gt_ptr), np.asarray(eligible))
    np.testing.assert_array_equal(_bits(mrr), _bits(rm))
    np.testing.assert_array_equal(_bits(auc), _bits(ra))
    return mrr, auc


def test_hand_built_rows():
    # g = 0: every entry ineligible
    mrr, auc = _check([-1, -1, -1], [0, 3], [10])
    assert mrr[0] == 0.0 and auc[0] == 0.0
    # M = g: nothing else to be ranked against
    mrr, auc = _check([2, 0, 1], [0, 3], [3])
    assert mrr[0] == 1.0 and auc[0] == 1.0
    # repeats count once: {4, 7} among 10
    mrr, auc = _check([7, 4, 7, 4, -1], [0, 5], [10])
    assert mrr[0] == np.float32(1.0 / 5.0)
    assert auc[0] == np.float32(1.0 - (4 + 6) / (2.0 * 8.0))
    # the best ranks and the worst
    mrr, auc = _check([0, 1, 2], [0, 3], [1000])
    assert mrr[0] == 1.0 and auc[0] == 1.0
    mrr, auc = _check([999, 998, 997], [0, 3], [1000])
    assert mrr[0] == np.float32(1.0 / 998.0) and auc[0] == 0.0
    # the largest catalogue an int32 rank can address
    big = 2 ** 31 - 1
    mrr, auc = _check([big - 1], [0, 1], [big])
    assert auc[0] == 0.0
    _check([big // 2, 5, big - 7], [0, 3], [big])


def test_one_row_among_many():
    rng = np.random.default_rng(1)
    n = 200
    cnt = rng.integers(1, 40, n)
    gp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    elig = rng.integers(40, 5000, n).astype(np.int32)
    rank = np.concatenate([rng.integers(-1, elig[i], cnt[i]) for i in range(n)]).astype(np.int32)
    rank[gp[7]:gp[8]] = rng.permutation(cnt[7])  # row 7: M = g
    elig[7] = cnt[7]
    rank[gp[9]:gp[10]] = -1                      # row 9: g = 0
    mrr, auc = _check(rank, gp, elig)
    assert auc[7] == 1.0 and mrr[9] == 0.0 and auc[9] == 0.0
    for i in (0, 7, 199):  # a row alone is the same row
        m1, a1 = fh.position_metrics(rank[gp[i]:gp[i + 1]], [0, cnt[i]], elig[i:i + 1])
        assert _bits(m1)[0] == _bits(mrr)[i] and _bits(a1)[0] == _bits(auc)[i]
    assert ((auc >= 0) & (auc <= 1) & (mrr >= 0) & (mrr <= 1)).all()


def test_argument_errors():
    lib = fh.load_library()
    P = fh._ptr
    rank = np.array([0, 1], np.int32)
    el = np.array([5, 5], np.int32)
    out = np.full(4, 7.0, np.float32)

    def call(rk, gp, e, n, mrr=out[:2], auc=out[2:]):
        gp = None if gp is None else np.asarray(gp, np.int64)
        return lib.frecsys_position_metrics(P(rk), P(gp), P(e), n, P(mrr), P(auc))

    assert call(rank, [0, 1, 2], el, 2) == fh.OK
    out[:] = 7.0
    assert call(rank, None, el, 2) == fh.ERR_INVALID
    assert call(rank, [0, 1, 2], el, -1) == fh.ERR_INVALID
    assert call(rank, [1, 1, 2], el, 2) == fh.ERR_INVALID          # gt_ptr[0] != 0
    assert call(rank, [0, 2, 1], el, 2) == fh.ERR_INVALID          # not monotone
    assert call(rank, [0, 0, 2], el, 2) == fh.ERR_INVALID          # a row with no ground truth
    assert call(None, [0, 1, 2], el, 2) == fh.ERR_INVALID
    assert call(rank, [0, 1, 2], None, 2) == fh.ERR_INVALID
    assert call(rank, [0, 1, 2], el, 2, mrr=None) == fh.ERR_INVALID
    assert call(rank, [0, 1, 2], el, 2, auc=None) == fh.ERR_INVALID
    assert call(np.array([0, -2], np.int32), [0, 1, 2], el, 2) == fh.ERR_INVALID
    assert call(np.array([0, 5], np.int32), [0, 1, 2], el, 2) == fh.ERR_INVALID  # rank = eligible
    # a rank with nothing eligible, in the second row
    assert call(rank, [0, 1, 2], np.array([5, 0], np.int32), 2) == fh.ERR_INVALID
    assert call(np.array([0, 1], np.int32), [0, 2], np.array([1], np.int32), 1) == fh.ERR_INVALID
    assert b"position_metrics" in lib.frecsys_last_error(None)
    assert (out == 7.0).all()                                      # nothing written
    assert call(None, [0], None, 0, mrr=None, auc=None) == fh.OK   # no rows
    with pytest.raises(fh.FrecsysError) as ei:
        fh.position_metrics([0], [0, 0, 1], [3, 3])
    assert ei.value.code == fh.ERR_INVALID


@pytest.mark.parametrize("exclude,mk", [(False, "none"), (True, "m70"), (True, "zero")])
def test_ranks64_against_recommend64_lists(exclude, mk):
    m, rows, dim = 257, 9, 20
    X, V, ptr, col, gp, gi = PR.inputs(m, rows, dim, "all", 41)
    mask = RR.grid_mask(m, mk, 41)
    S, items, _ = RR.recommend64(X, V, ptr, col, None, m, exclude, mask)
    rank, elig = PR.ranks64(S, gp, gi)
    np.testing.assert_array_equal(elig, (items >= 0).sum(axis=1))
    for i in range(rows):
        g = gi[gp[i]:gp[i + 1]]
        r = rank[gp[i]:gp[i + 1]]
        listed = r >= 0
        # the item at position rank is the item
        np.testing.assert_array_equal(items[i, r[listed]], g[listed])
        assert not set(g[~listed].tolist()) & set(items[i].tolist())
    assert (rank >= 0).any() or mk == "zero"


def test_plan_covers_every_pair():
    cases = [c[:7] for c in PR.plan()]
    for a, b in itertools.combinations(range(7), 2):
        seen = {(c[a], c[b]) for c in cases}
        want = set(itertools.product(PR.PLAN_AXES[a], PR.PLAN_AXES[b]))
        assert want <= seen, (a, b, sorted(want - seen, key=repr))
    assert PR.plan() == PR.plan()  # deterministic
    assert len(PR.plan_main()) <= 80
    # the thresholds straddle the LDS limit with distinct ids where the items allow
    gp, gi = PR.ground_truth(1025, 4, "L+1", [0, 0, 0, 0, 0], [], 3)
    assert (np.diff(gp) == PR.LDS_THRESHOLDS + 1).all()
    assert len(set(gi[gp[0]:gp[1]].tolist())) == PR.LDS_THRESHOLDS + 1


def test_plan_inputs_hold_ties_and_ineligible_ground_truth():
    X, V, ptr, col, gp, gi = PR.inputs(1025, 65, 5, "L+1", 5001)
    mask = RR.grid_mask(1025, "m70", 5001)
    S, _, _ = RR.recommend64(X, V, ptr, col, None, 1, True, mask)
    rank, elig = PR.ranks64(S, gp, gi)
    assert (rank == -1).any() and (rank >= 0).any()
    fin = S[0][np.isfinite(S[0])]
    assert len(np.unique(fin)) < len(fin) / 4  # heavy ties
    assert (np.diff(gp)[4::5] == PR.LDS_THRESHOLDS + 2).all()  # the repeated entry
