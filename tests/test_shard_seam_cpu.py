"""The shard fixtures' contract (tests/shard_data.py), checked without a GPU:
the bounds partition_rows gives them, the properties of an nnz-balanced split
in general, what each world's shards are made of, on which side of the 70 %
row-subset rule the shards fall, and the fp32 C oracle alone against float64
on the skew fixture -- at most a quarter of the 1e-4 row bar, as on the seam
fixture (test_seam_cpu.py).
"""
import numpy as np
import pytest

import seam_data as S
import shard_data as D
from conftest import rel_rows

fh = pytest.importorskip("frecsys_hip")

ORACLE_CAP = 2.5e-5  # a quarter of TOL_ROW = 1e-4
DIMS = (8, 64, 256, 500, 1000)


@pytest.mark.parametrize("fixture,world", list(D.BOUNDS))
def test_bounds_are_the_listed_ones(fixture, world):
    """The C function, its restatement and the constants, in both orientations."""
    d = D.fixture_data(fixture)
    for ptr in (d["user"][2], d["item"][4]):
        np.testing.assert_array_equal(np.diff(ptr), [len(x) for x in d["sd"].hists])
        want = D.BOUNDS[fixture, world]
        assert tuple(D.partition(ptr, world)) == want
        assert tuple(int(x) for x in fh.partition(ptr, world)) == want
    assert world in D.WORLDS[fixture]


def test_other_side_of_the_seam_fixture_splits_evenly():
    """No seam there: 704 rows of h = 15..58."""
    ip = D.fixture_data("seam")["user"][4]
    h = np.diff(ip)
    assert (h.min(), h.max()) == (15, 58)
    b = D.partition(ip, 8)
    assert b == [0, 89, 177, 265, 351, 442, 530, 618, 704]
    assert [int(x) for x in fh.partition(ip, 8)] == b


def _random_row_ptrs():
    rng = np.random.default_rng(11)
    out = [("all_idle", np.zeros(8, np.int64)), ("one_entity", np.array([0, 17], np.int64)),
           ("one_idle_entity", np.array([0, 0], np.int64))]
    for i in range(40):
        n = int(rng.integers(1, 60))
        h = rng.integers(0, 50, n)
        h[rng.random(n) < 0.3] = 0
        if i % 4 == 0:
            h[int(rng.integers(0, n))] = int(rng.integers(500, 5000))  # one heavy entity
        if i % 8 == 1:
            h[n // 2:] = 0  # an idle tail
        out.append((f"random{i}", np.concatenate([[0], np.cumsum(h)]).astype(np.int64)))
    return out


@pytest.mark.parametrize("name,ptr", _random_row_ptrs(), ids=[n for n, _ in _random_row_ptrs()])
def test_partition_properties(name, ptr):
    n = len(ptr) - 1
    nnz = int(ptr[-1])
    for parts in (1, 2, 3, 8, n + 1, 2 * n + 3):
        b = [int(x) for x in fh.partition(ptr, parts)]
        assert b == D.partition(ptr, parts), (name, parts)
        assert len(b) == parts + 1 and b[0] == 0 and b[-1] == n
        assert all(x <= y for x, y in zip(b, b[1:]))
        for r in range(1, parts):
            if b[r] in (0, n):
                continue
            # an interior start: the first row whose prefix reaches the target
            target = nnz * r // parts
            h_before = int(ptr[b[r]] - ptr[b[r] - 1])
            assert target <= int(ptr[b[r]]) < target + max(h_before, 1), (name, parts, r)


def _kinds_of(fixture, world, quirk, threshold):
    ptr = D.solved_ptr(fixture)
    h = np.diff(ptr)
    return D.shard_kinds(h, S.h_eff(h, quirk), D.BOUNDS[fixture, world], threshold)


def test_fixture_properties():
    """What the right-hand column of the bounds table says, from h and h_eff."""
    ptr = D.solved_ptr("seam")
    h = np.diff(ptr)
    found = set()
    for fixture, world in D.BOUNDS:
        for quirk in (False, True):
            for thr in D.HSPACE_MAX_H.values():
                for k in _kinds_of(fixture, world, quirk, thr):
                    found |= k
    D.check_coverage(found)
    # seam, W = 3: shard 1 holds h = 384..513 only
    lo, hi = D.shards(D.BOUNDS["seam", 3])[1]
    assert (h[lo:hi].min(), h[lo:hi].max()) == (384, 513)
    for thr in D.HSPACE_MAX_H.values():
        assert _kinds_of("seam", 3, False, thr)[1] == {"above"}
        assert _kinds_of("seam", 3, False, thr)[0] == {"straddle"}
    assert (S.h_eff(h[lo:hi], True) <= 640).all() and (h[lo:hi] <= 513).all()  # the wide bucket
    # seam, W = 8: shard 0 is h <= 224, shards 1-4 lie above both thresholds
    # but for h = 225..256 of shard 1 at the wide dims, shard 5 is mixed,
    # shards 6 and 7 hold fillers and idle rows
    k8 = _kinds_of("seam", 8, False, 224)
    assert k8[0] == {"below"} and h[:23].max() == 224
    assert all(k == {"above"} for k in k8[1:5])
    assert k8[5] == {"straddle"}
    labels = D.fixture_data("seam")["sd"].labels
    for r in (6, 7):
        lo, hi = D.shards(D.BOUNDS["seam", 8])[r]
        assert "filler" in labels[lo:hi] and "idle" in labels[lo:hi]
    assert _kinds_of("seam", 8, False, 256)[1] == {"straddle"}
    # seam, W = 16: shards of two and three entities
    b16 = D.BOUNDS["seam", 16]
    small = {tuple(int(x) for x in h[lo:hi]) for lo, hi in D.shards(b16) if hi - lo <= 3}
    assert {(447, 448), (383, 384, 385), (415, 416, 417)} <= small
    # skew: one heavy entity per shard | an idle-only last shard | an empty
    # shard, then an idle-only one | three empty shards in a row, twice
    hs = np.asarray(D.SKEW_H)
    np.testing.assert_array_equal(np.diff(D.solved_ptr("skew")), hs)
    assert [int((hs[lo:hi] >= 600).sum()) for lo, hi in D.shards(D.BOUNDS["skew", 2])] == [1, 1]
    assert _kinds_of("skew", 3, False, 224)[2] == {"idle", "small"}
    k4 = _kinds_of("skew", 4, False, 224)
    assert k4[1] == {"empty"} and k4[3] == {"idle", "small"}
    k8s = _kinds_of("skew", 8, False, 224)
    assert [("empty" in k) for k in k8s] == [False, True, True, True, False, True, True, False]
    assert k8s[7] == {"idle", "small"}


def test_subset_sizes():
    """Both sides of the 70 % rule at W = 8 and at W = 16 at the thresholds 224
    and 256, so the subset pass and the plain pass both run in
    test_shard_seam_gpu.py.  At the limits the wide dims really use (320 for
    the users and 512 for the items at Dp = 512, 512 at Dp = 1024) W = 8 has
    a subset shard only at 320 and W = 16 at both: d = 500 runs both passes,
    d = 1000 (W = 3 and 8 only) the plain one alone."""
    for key, quirk in (("ials_user", False), ("weighted_v_quirk", True)):
        c = S.seam_case(key, 8)
        wide = {320: set(), 512: set()}
        for world in (8, 16):
            for max_h in (224, 256, 320, 512):
                sizes = [D.subset_rows(c, lo, hi, max_h)
                         for lo, hi in D.shards(D.BOUNDS["seam", world])]
                with_hs = [rows for n, rows in sizes if n > 0]
                print(f"{key} W={world} max_h={max_h}: (entities, rows) {sizes}")
                if max_h in wide:
                    wide[max_h] |= {D.takes_subset(r) for r in with_hs}
                    continue
                assert any(D.takes_subset(r) for r in with_hs), (key, world, max_h)
                assert any(not D.takes_subset(r) for r in with_hs), (key, world, max_h)
        assert wide == {320: {True, False}, 512: {True, False}}
    assert D.takes_subset(492) and not D.takes_subset(493)  # 0.7 * 704 = 492.8


def test_skew_history_space_entities_do_not_read_row_zero():
    """The history-space kernels load row 0 of the rotated table for the
    padding rows of a tile.  On the skew fixture no history-space entity reads
    row 0 and every shard takes the subset pass, so the row is rotated only
    because hspace_rows always lists it: the case that showed it missing."""
    c = D.case("skew", "ials_user", 64)
    short = [e for e in range(len(c.h)) if 0 < c.h[e] <= 224]
    assert [int(c.h[e]) for e in short] == [3, 1, 2, 33]
    read = set(np.concatenate([c.col[c.ptr[e]:c.ptr[e + 1]] for e in short]).tolist())
    assert 0 not in read and len(read) == 39
    assert D.takes_subset(D.subset_rows(c, 0, 10, 224)[1])
    assert D.subset_rows(c, 0, 10, 224) == (4, 40)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("key", list(S.KINDS))
def test_oracle_within_a_quarter_of_the_bar_on_skew(key, dim):
    c = D.case("skew", key, dim)
    np.testing.assert_array_equal(c.h, D.SKEW_H)
    ref = S.reference(c)
    out = S.oracle_step(c)
    live = c.h > 0
    err = rel_rows(out[live], ref[live])
    worst = np.nonzero(live)[0][int(err.argmax())]
    print(f"skew oracle vs float64: {key} d={dim} max {err.max():.2e} (h = {c.h[worst]})")
    assert err.max() < ORACLE_CAP, (err.max(), int(c.h[worst]))
    np.testing.assert_array_equal(out[~live], c.E[~live])
    np.testing.assert_array_equal(ref[~live], c.E[~live].astype(np.float64))
    if c.kind == 1:  # omega = 0 at index 6 (h = 33)
        assert c.entity_weight[6] == 0 and not ref[6].any() and not out[6].any()


def test_skew_case_is_not_the_seam_case():
    """The two fixtures share keys and dims: their references must not."""
    a, b = S.seam_case("ials_user", 8), D.case("skew", "ials_user", 8)
    assert S.reference(a).shape == (104, 8) and S.reference(b).shape == (10, 8)
    assert S.reference(S.seam_case("ials_user", 8)) is S.reference(a)
