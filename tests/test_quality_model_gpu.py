"""Model.evaluate_quality / evaluate_quality_fold_in / list_quality /
item_self_information (include/frecsys_model.h) on the ML-1M golden files: iALS
at dim 64 after two epochs.

The per-row values are Context.rank_quality's / lists_quality's of the same
rows, byte for byte; the summary lines are their means (double sums in row
order), frecsys_exposure_summary of the exposure rows and Model.evaluate's
summary.  lam = 1 gives what pool = None gives.  Sanity, no tolerance: ILD@20 at
lam = 0.3 is not below ILD@20 at lam = 1 in the mean over the queried users --
by the library's values and by the pairwise float64 reference of
tests/quality_ref.py on the fetched lists.  Serve-only and argument refusals:
the code and the exact message of a single defect, before any projection.
"""
import numpy as np
import pytest

import quality_ref as Q

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

DIM, KS, POOL = 64, (5, 20, 10), 200
INVALID = fh.ERR_INVALID


@pytest.fixture(scope="module")
def model(ml1m):
    tr, _, _ = ml1m
    m = fh.Model("ials", tr.users, tr.items, dim=DIM, stdev=0.1, seed=1, l2_reg=0.003,
                 l2_reg_exp=1.0, uobs_weight=0.1, print_train_stats=False)
    m.initialize()
    m.train(2)
    yield m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _truth(n, ni, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 9, n)
    gp = np.concatenate([[0], np.cumsum(g)]).astype(np.int64)
    return gp, rng.integers(0, ni, gp[-1]).astype(np.int32)


def _same_rows(got, want, keys=("ild", "novelty", "recall", "ndcg")):
    for key in keys:
        assert (got.get(key) is None) == (want.get(key) is None), key
        if want.get(key) is not None:
            np.testing.assert_array_equal(_bits(got[key]), _bits(want[key]), err_msg=key)
    np.testing.assert_array_equal(got["exposure"], want["exposure"])


def _check_summary(ev, n, mask=None):
    for q in range(len(ev["k_list"])):
        for name in ("ild", "novelty"):
            if ev[name] is None:
                assert ev["mean_" + name] is None
                continue
            s = 0.0
            for x in ev[name][:, q]:     # row order, in double
                s += float(x)
            assert ev["mean_" + name][q] == s / n, (name, q)
        want = fh.exposure_summary(ev["exposure"][q], mask)
        assert want == Q.summary_exact(ev["exposure"][q], mask)
        assert (ev["coverage"][q], ev["gini"][q]) == (want["coverage"], want["gini"])


def test_item_self_information(model, ml1m):
    tr, _, _ = ml1m
    w = model.item_self_information()
    h = np.bincount(tr.items, minlength=model.n_items)
    want = (-np.log2(np.maximum(h, 1) / model.n_users)).astype(np.float32)
    assert w.dtype == np.float32 and w.shape == (model.n_items,)
    np.testing.assert_array_equal(w, want)
    assert np.isfinite(w).all() and w.min() >= 0


def test_trained_users(model):
    m = model
    ctx = m.context()
    w = m.item_self_information()
    rng = np.random.default_rng(31)
    users = np.concatenate([[0, m.n_users - 1], rng.permutation(m.n_users)[:300]])
    gt = _truth(len(users), m.n_items, 32)
    mask = (rng.random(m.n_items) < 0.5).astype(np.uint8)
    plain = m.evaluate_quality(users, KS, gt=gt, item_weight=w)
    _same_rows(plain, ctx.rank_quality(fh.SIDE_USER, KS, rows=users, item_weight=w, gt=gt))
    _check_summary(plain, len(users))
    ev = m.evaluate(users, gt[0], gt[1], k_list=KS)
    for key in ("recall", "ndcg", "mean_recall", "mean_ndcg", "recall_cvar", "ndcg_cvar"):
        np.testing.assert_array_equal(_bits(plain[key]), _bits(ev[key]), err_msg=key)
    # the MMR stage in front, the history kept, a mask; no weights, no ground truth
    div = m.evaluate_quality(users, KS, pool=POOL, lam=0.5, exclude_seen=False, item_mask=mask)
    assert div["novelty"] is None and "recall" not in div
    _same_rows(div, ctx.rank_quality(fh.SIDE_USER, KS, rows=users, pool=POOL, lam=0.5,
                                     exclude_history=False, item_mask=mask))
    _check_summary(div, len(users), mask)
    lists = m.recommend_diverse(users, max(KS), pool=POOL, lam=0.5, exclude_history=False,
                                item_mask=mask)[0]
    lq = m.list_quality(lists, KS, item_weight=w, item_mask=mask)
    _same_rows(lq, ctx.lists_quality(lists, KS, w))
    _check_summary(lq, len(users), mask)
    np.testing.assert_array_equal(_bits(lq["ild"]), _bits(div["ild"]))
    np.testing.assert_array_equal(lq["exposure"], div["exposure"])
    # lam = 1 is the plain top-K
    _same_rows(m.evaluate_quality(users, KS, pool=POOL, lam=1.0, gt=gt, item_weight=w), plain)
    # diversity bought: ILD@20 at lam = 0.3 against lam = 1
    low = m.evaluate_quality(users, KS, pool=POOL, lam=0.3)
    q20 = KS.index(20)
    V = ctx.get_embeddings(fh.SIDE_ITEM)
    top_lists = m.recommend(users, 20)[0]
    low_lists = m.recommend_diverse(users, 20, pool=POOL, lam=0.3)[0]
    ref_top = Q.quality64(V, top_lists, (20,))[0].mean()
    ref_low = Q.quality64(V, low_lists, (20,))[0].mean()
    print(f"mean ILD@20: lam=1 {plain['mean_ild'][q20]:.4f} (float64 pairwise {ref_top:.4f}), "
          f"lam=0.3 {low['mean_ild'][q20]:.4f} ({ref_low:.4f})")
    assert low["mean_ild"][q20] >= plain["mean_ild"][q20] and ref_low >= ref_top
    assert Q.close(low["ild"][:, q20], Q.quality64(V, low_lists, (20,))[0][:, 0]) <= 1.0


def test_fold_in_users(model, ml1m):
    m = model
    _, vt, _ = ml1m
    _, ep, ec = vt.compact_users()
    n = 200
    ep, ec = ep[:n + 1], ec[:ep[n]]
    w = m.item_self_information()
    gt = _truth(n, m.n_items, 33)
    got = m.evaluate_quality_fold_in(ep, ec, KS, pool=80, lam=0.5, gt=gt, item_weight=w)
    # the projected rows stay in the EVAL side
    want = m.context().rank_quality(fh.SIDE_EVAL, KS, rows=np.arange(n), pool=80, lam=0.5,
                                    item_weight=w, gt=gt)
    _same_rows(got, want)
    _check_summary(got, n)
    lists = m.recommend_diverse_fold_in(ep, ec, max(KS), pool=80, lam=0.5)[0]
    host = fh.list_quality(m.context().get_embeddings(fh.SIDE_ITEM), lists, KS, w)
    assert Q.close(got["ild"], host[0]) <= 1.0 and Q.close(got["novelty"], host[1]) <= 1.0
    np.testing.assert_array_equal(got["exposure"], host[2])
    empty = m.evaluate_quality_fold_in(np.zeros(1, np.int64), np.zeros(0, np.int32), KS)
    assert empty["ild"].shape == (0, 3) and empty["exposure"].sum() == 0


def test_serve_only(model, tmp_path):
    m = model
    users = np.arange(0, m.n_users, 61)
    w = m.item_self_information()
    want = m.evaluate_quality(users, KS, pool=80, lam=0.5, item_weight=w, exclude_seen=False)
    path = str(tmp_path / "serve.frm")
    m.save(path, include_data=False)
    b = fh.Model.load(path)
    try:
        _same_rows(b.evaluate_quality(users, KS, pool=80, lam=0.5, item_weight=w,
                                      exclude_seen=False), want)
        with pytest.raises(fh.FrecsysError) as e:
            b.evaluate_quality(users, KS)
        assert str(e.value) == (f"frecsys error {INVALID}: frecsys_model_evaluate_quality: the "
                                "model was loaded without training tuples (serve-only): no "
                                "training and no exclude_seen")
        with pytest.raises(fh.FrecsysError) as e:
            b.item_self_information()
        assert e.value.code == INVALID
        hp, hi = np.array([0, 2], np.int64), np.array([1, 3], np.int32)
        got = b.evaluate_quality_fold_in(hp, hi, KS)        # the history it is given
        assert got["exposure"][:, [1, 3]].sum() == 0 and got["exposure"][1].sum() == 20
    finally:
        b.close()


def test_defects(model):
    """One call per single defect through the C-ABI: the code and the message."""
    m = model
    lib, P = m.lib, fh._ptr
    ni = m.n_items
    n = 2
    base = dict(users=np.array([0, 5], np.int64), n=n, k_list=np.array([3, 7], np.int32), nk=2,
                pool=0, lam=0.5, raw=0, weight=np.ones(ni, np.float32),
                gt_ptr=np.array([0, 1, 3], np.int64), gt_items=np.array([2, 0, 4], np.int32),
                alpha=np.array([0.5], np.float32), na=1, exc=1, mask=None,
                ild=np.zeros(n * 2, np.float32), nov=np.zeros(n * 2, np.float32),
                rec=np.zeros(n * 2, np.float32), ndcg=np.zeros(n * 2, np.float32),
                ex=np.zeros(2 * ni, np.int64), summary=np.zeros(16, np.float64),
                hist_ptr=np.array([0, 2, 3], np.int64), hist_items=np.array([1, 3, 0], np.int32))

    def call(fold, **over):
        a = dict(base, **over)
        tail = [P(a["k_list"]), a["nk"], a["pool"], a["lam"], a["raw"], P(a["weight"]),
                P(a["gt_ptr"]), P(a["gt_items"]), P(a["alpha"]), a["na"], a["exc"], P(a["mask"]),
                P(a["ild"]), P(a["nov"]), P(a["rec"]), P(a["ndcg"]), P(a["ex"]), P(a["summary"])]
        if fold:
            rc = lib.frecsys_model_evaluate_quality_fold_in(m.h, P(a["hist_ptr"]),
                                                            P(a["hist_items"]), a["n"], *tail)
        else:
            rc = lib.frecsys_model_evaluate_quality(m.h, P(a["users"]), a["n"], *tail)
        return rc, lib.frecsys_model_last_error().decode()

    bad_w = base["weight"].copy()
    bad_w[9] = -np.inf
    cases = [
        (dict(k_list=None), "k_list must hold 1 to 32 cut-offs"),
        (dict(nk=33), "k_list must hold 1 to 32 cut-offs"),
        (dict(k_list=np.array([3, 0], np.int32)), "cut-offs must be in [1, 1024]"),
        (dict(k_list=np.array([3, 1025], np.int32)), "cut-offs must be in [1, 1024]"),
        (dict(ild=None, nov=None, ex=None, rec=None, ndcg=None, weight=None, gt_ptr=None,
              gt_items=None), "null outputs"),
        (dict(weight=None), "novelty needs item_weight"),
        (dict(nov=None), "item_weight without a novelty output"),
        (dict(weight=bad_w), "item_weight[9] is not finite"),
        (dict(pool=-1), "pool must be 0 or in [1, 1024]"),
        (dict(pool=1025), "pool must be 0 or in [1, 1024]"),
        (dict(pool=6), "cut-offs must not exceed pool"),
        (dict(pool=8, lam=1.5), "lam must be in [0, 1]"),
        (dict(pool=8, lam=float("nan")), "lam must be in [0, 1]"),
        (dict(pool=8, raw=2), "raw_scores must be 0 or 1"),
        (dict(raw=1), "raw_scores without a pool"),
        (dict(na=-1), "bad alpha_list"),
        (dict(gt_ptr=None, gt_items=None), "recall / ndcg need a ground truth"),
        (dict(ndcg=None), "a ground truth needs recall and ndcg"),
        (dict(gt_ptr=np.array([1, 1, 3], np.int64)), "bad arguments (n < 0, gt_ptr)"),
        (dict(gt_items=None), "null gt_items"),
        (dict(gt_ptr=np.array([0, 0, 3], np.int64)),
         "gt_ptr not monotone or no ground truth at row 0"),
        (dict(gt_items=np.array([2, ni, 4], np.int32)), f"ground-truth id {ni} out of range"),
    ]
    for fold in (False, True):
        who = "frecsys_model_evaluate_quality" + ("_fold_in" if fold else "")
        assert call(fold)[0] == fh.OK
        assert call(fold, exc=0)[0] == fh.OK
        for over, msg in cases:
            rc, err = call(fold, **over)
            assert (rc, err) == (INVALID, f"{who}: {msg}"), (fold, list(over), rc, err)
        # a negative n: the history CSR's check, or the ground truth's own words
        assert call(fold, n=-1) == \
            (INVALID, f"{who}: bad arguments" + ("" if fold else " (n < 0, gt_ptr)"))
    assert call(False, users=None) == (INVALID, "frecsys_model_evaluate_quality: bad arguments")
    assert call(True, hist_items=np.array([1, ni, 0], np.int32)) == \
        (INVALID, f"frecsys_model_evaluate_quality_fold_in: item id {ni} out of range")
    # a rejected fold-in call projects nothing: EVAL still holds the last good call's rows
    assert call(True)[0] == fh.OK
    three = dict(n=3, hist_ptr=np.array([0, 1, 3, 4], np.int64),
                 hist_items=np.array([0, 1, 2, 3], np.int32),
                 gt_ptr=np.array([0, 1, 2, 3], np.int64), ild=np.zeros(6, np.float32),
                 nov=np.zeros(6, np.float32), rec=np.zeros(6, np.float32),
                 ndcg=np.zeros(6, np.float32))
    assert call(True, **three)[0] == fh.OK
    assert call(True)[0] == fh.OK
    assert call(True, **dict(three, pool=8, lam=float("nan")))[0] == INVALID
    assert m.context().csr_row_lengths(fh.SIDE_EVAL, n=2).tolist() == [2, 1]
    # caller lists
    L = np.zeros((2, 8), np.int32)
    out = np.zeros(4, np.float32)

    def lists(lists_=L, n_=2, list_k=8, ks=base["k_list"], ild=out):
        rc = lib.frecsys_model_list_quality(m.h, P(lists_), n_, list_k, P(ks), 2, None, None,
                                            P(ild), None, None, None)
        return rc, lib.frecsys_model_last_error().decode()

    who = "frecsys_model_list_quality: "
    assert lists()[0] == fh.OK
    assert lists(lists_=None) == (INVALID, who + "bad arguments")
    assert lists(n_=-1) == (INVALID, who + "bad arguments")
    assert lists(list_k=0) == (INVALID, who + "bad arguments")
    assert lists(ks=np.array([3, 9], np.int32)) == (INVALID, who + "cut-offs must be in [1, 8]")
    assert lists(ild=None) == (INVALID, who + "null outputs")
    assert lists(lists_=np.full((2, 8), ni, np.int32)) == \
        (INVALID, f"lists_quality: item id {ni} out of range")
