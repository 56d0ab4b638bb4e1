"""frecsys_sample_negatives (the host sampler of sampled evaluation) against
the pure-Python restatement of tests/sampled_ref.py, and the surface of the
feature, checked without a GPU.

test_grid_equals_reference      neg_count and negatives (draw order) equal on
                                the grid of sampled_ref.plan().
test_whole_pool_boundaries      rows with E in {2n-1, 2n, 2n+1} and
                                64 E in {M-1, M, M+1}: both sides of each rule.
test_repeats_inside_and_across_blocks
                                129 items, 60 negatives: the reference met
                                repeats inside a block of 64 draws and across
                                blocks, and the library agrees draw for draw.
test_row_independent            a row's sample does not depend on the others.
test_invalid_arguments          every FRECSYS_ERR_INVALID case, outputs
                                untouched.
test_surface                    headers, exported symbols, Python names.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sampled_ref as SR
from conftest import ROOT

fh = pytest.importorskip("frecsys_hip")

N_ROWS = 24


def _run(n_items, mask, rows, hist, gp, gi, n_neg, seed):
    return fh.sample_negatives(n_items, gp, gi, n_neg, seed, rows=rows,
                               hist_ptr=None if hist is None else hist[0],
                               hist_items=None if hist is None else hist[1], item_mask=mask)


def test_plan_covers_the_grid():
    p = SR.plan()
    assert {(c[0], c[1]) for c in p} >= {(m, n) for m in SR.GRID_ITEMS for n in SR.GRID_NEG}
    assert {(c[0], c[2]) for c in p} == {(m, k) for m in SR.GRID_ITEMS for k in SR.GRID_MASKS}
    for m in SR.GRID_ITEMS:
        mine = [c for c in p if c[0] == m]
        assert {c[3] for c in mine} == {False, True}
        assert {c[4] for c in mine} == set(SR.GRID_SEEDS)
        assert {c[5] for c in mine} == set(SR.GRID_ROWMODES)


@pytest.mark.parametrize("n_items,n_neg,mk,with_hist,seed,row_mode,fseed", SR.plan())
def test_grid_equals_reference(n_items, n_neg, mk, with_hist, seed, row_mode, fseed):
    mask, rows, hist, gp, gi, _ = SR.case(n_items, N_ROWS, mk, with_hist, row_mode, fseed)
    ref = SR.sample(n_items, mask, rows, hist, gp, gi, n_neg, seed)
    cnt, neg = _run(n_items, mask, rows, hist, gp, gi, n_neg, seed)
    assert neg.shape == (N_ROWS, n_neg)
    np.testing.assert_array_equal(cnt, ref["neg_count"])
    np.testing.assert_array_equal(neg, ref["negatives"])
    for i in np.nonzero(~ref["whole"])[0]:   # distinct ids of the pool, in draw order
        h = hist[1][hist[0][i]:hist[0][i + 1]] if hist is not None else []
        pool = set(SR.pool_of(n_items, mask, h, gi[gp[i]:gp[i + 1]]).tolist())
        assert len(set(neg[i].tolist())) == n_neg and set(neg[i].tolist()) <= pool
    if rows is not None:   # equal r, equal ground truth and history: an equal sample
        assert rows[N_ROWS // 2] == rows[0] and rows[-1] == rows[1] or row_mode == "ordered"
        gt = [tuple(sorted(set(gi[gp[i]:gp[i + 1]].tolist()))) for i in range(N_ROWS)]
        same = [(i, j) for i in range(N_ROWS) for j in range(i)
                if rows[i] == rows[j] and gt[i] == gt[j]]
        assert same or row_mode == "ordered"
        for i, j in same:
            np.testing.assert_array_equal(neg[i], neg[j])


def _boundary_rows(M, n_items, mask, targets):
    """One row per target pool size E: ground truth one id of D, history a
    prefix of the rest of D so that E ids stay."""
    D = np.arange(n_items) if mask is None else np.nonzero(mask)[0]
    assert len(D) == M
    gt, hs = [], []
    for E in targets:
        gt.append(D[:1])
        hs.append(D[1:M - E])
        assert M - 1 - len(hs[-1]) == E
    gp = np.arange(len(targets) + 1, dtype=np.int64)
    hp = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int64)
    return gp, np.concatenate(gt).astype(np.int32), (hp, np.concatenate(hs).astype(np.int32))


def test_whole_pool_boundaries():
    # 2 n_neg against E, 64 E >= M throughout
    n_neg, M = 10, 200
    gp, gi, hist = _boundary_rows(M, M, None, (2 * n_neg - 1, 2 * n_neg, 2 * n_neg + 1))
    ref = SR.sample(M, None, None, hist, gp, gi, n_neg, 3)
    assert ref["E"].tolist() == [19, 20, 21] and ref["whole"].tolist() == [True, False, False]
    cnt, neg = _run(M, None, None, hist, gp, gi, n_neg, 3)
    np.testing.assert_array_equal(cnt, [19, 10, 10])
    np.testing.assert_array_equal(neg, ref["negatives"])
    assert (neg[0] == -1).all() and (neg[1:] >= 0).all()
    # 64 E against M (E = 4 >= 2 n_neg), without a mask and with M ones in 5000
    for M in (255, 256, 257):
        for n_items in (M, 5000):
            mask = None
            if n_items != M:
                mask = np.zeros(n_items, np.uint8)
                mask[np.random.default_rng(M).permutation(n_items)[:M]] = 1
            gp, gi, hist = _boundary_rows(M, n_items, mask, (4, 4))
            ref = SR.sample(n_items, mask, None, hist, gp, gi, 2, 1)
            assert ref["M"] == M and ref["E"].tolist() == [4, 4]
            assert 64 * 4 - M in (1, 0, -1)
            assert ref["whole"].tolist() == [64 * 4 < M] * 2
            cnt, neg = _run(n_items, mask, None, hist, gp, gi, 2, 1)
            np.testing.assert_array_equal(cnt, [4, 4] if 64 * 4 < M else [2, 2])
            np.testing.assert_array_equal(neg, ref["negatives"])


def test_repeats_inside_and_across_blocks():
    n_items, n_neg, n = 129, 60, 8
    gp = np.arange(n + 1, dtype=np.int64)
    gi = (16 * np.arange(n)).astype(np.int32)
    ref = SR.sample(n_items, None, None, None, gp, gi, n_neg, 7)
    assert not ref["whole"].any() and (ref["E"] == 128).all()
    assert ref["in_block"] > 0 and ref["across_blocks"] > 0, ref
    assert ref["draws"] > 64 * n   # every row went into a second block
    cnt, neg = _run(n_items, None, None, None, gp, gi, n_neg, 7)
    np.testing.assert_array_equal(cnt, np.full(n, n_neg))
    np.testing.assert_array_equal(neg, ref["negatives"])


def test_row_independent():
    n_items, n_neg = 5000, 100
    mask, rows, hist, gp, gi, _ = SR.case(n_items, N_ROWS, "m70", True, "shuffled", 77)
    cnt, neg = _run(n_items, mask, rows, hist, gp, gi, n_neg, 5)
    keep = [3, 17, 4, 4, 0, 23]
    sp = np.concatenate([[0], np.cumsum(gp[np.array(keep) + 1] - gp[keep])]).astype(np.int64)
    si = np.concatenate([gi[gp[i]:gp[i + 1]] for i in keep])
    hs = [hist[1][hist[0][i]:hist[0][i + 1]] for i in keep]
    hp = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int64)
    c2, n2 = _run(n_items, mask, rows[keep], (hp, np.concatenate(hs)), sp, si, n_neg, 5)
    np.testing.assert_array_equal(c2, cnt[keep])
    np.testing.assert_array_equal(n2, neg[keep])
    c3, n3 = _run(n_items, mask, rows, hist, gp, gi, n_neg, 6)   # another seed, another sample
    assert (n3 != neg).any()
    np.testing.assert_array_equal(c3, cnt)


def test_invalid_arguments():
    lib = fh.load_library()
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    gp, gi = np.array([0, 1, 3], np.int64), np.array([1, 2, 3], np.int32)
    hp, hi = np.array([0, 1, 1], np.int64), np.array([4], np.int32)
    rows = np.array([1, 0], np.int64)
    ok = dict(n_items=10, mask=None, rows=rows, n=2, hp=hp, hi=hi, gp=gp, gi=gi, n_neg=2, seed=1)

    def call(**kw):
        a = dict(ok, **kw)
        cnt = np.full(2, -7, np.int32)
        neg = np.full(4, -7, np.int32)
        rc = lib.frecsys_sample_negatives(a["n_items"], P(a["mask"]), P(a["rows"]), a["n"],
                                          P(a["hp"]), P(a["hi"]), P(a["gp"]), P(a["gi"]),
                                          a["n_neg"], a["seed"],
                                          None if a.get("no_cnt") else P(cnt), P(neg))
        return rc, cnt, neg

    rc, cnt, neg = call()
    assert rc == fh.OK and cnt.tolist() == [2, 2] and (neg >= 0).all()
    bad = [dict(n_items=0), dict(n_items=2 ** 31), dict(n=-1), dict(n_neg=-1),
           dict(n=2 ** 62, n_neg=4), dict(rows=np.array([0, -1], np.int64)), dict(no_cnt=True),
           dict(gp=None), dict(gi=None), dict(hp=None), dict(hi=None),
           dict(hp=np.array([-1, 0, 1], np.int64)), dict(hp=np.array([0, 1, 0], np.int64)),
           dict(gp=np.array([1, 2, 3], np.int64)), dict(gp=np.array([0, 2, 1], np.int64)),
           dict(gp=np.array([0, 0, 3], np.int64)), dict(gi=np.array([1, 2, 10], np.int32)),
           dict(gi=np.array([1, -1, 3], np.int32))]
    for kw in bad:
        rc, cnt, neg = call(**kw)
        assert rc == fh.ERR_INVALID, kw
        assert (cnt == -7).all() and (neg == -7).all(), kw
        assert b"sample_negatives" in lib.frecsys_last_error(None)
    # an empty history needs no hist_items; no rows: nothing is touched
    rc, cnt, neg = call(hp=np.zeros(3, np.int64), hi=None)
    assert rc == fh.OK and cnt.tolist() == [2, 2]
    rc, cnt, neg = call(n=0, gp=None, gi=None)
    assert rc == fh.OK and (cnt == -7).all() and (neg == -7).all()
    # negatives may be NULL
    cnt = np.zeros(2, np.int32)
    assert lib.frecsys_sample_negatives(10, None, None, 2, None, None, P(gp), P(gi), 2, 1, P(cnt),
                                        None) == fh.OK
    assert cnt.tolist() == [2, 2]
    with pytest.raises(fh.FrecsysError) as ei:
        fh.sample_negatives(10, gp, gi, -1)
    assert ei.value.code == fh.ERR_INVALID


def _declared(path):
    txt = open(os.path.join(ROOT, "include", path)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r" T (frecsys_\w+)", out))


CORE = ("frecsys_sample_negatives", "frecsys_rank_candidates_metrics", "frecsys_sampled_metrics")
MODEL = ("frecsys_model_evaluate_candidates", "frecsys_model_evaluate_candidates_fold_in",
         "frecsys_model_evaluate_sampled", "frecsys_model_evaluate_sampled_fold_in")


def test_surface():
    core, model = _declared("frecsys_hip.h"), _declared("frecsys_model.h")
    assert re.search(r"int frecsys_sample_negatives\(int64_t n_items,\s*const uint8_t\* item_mask,"
                     r"\s*const int64_t\* row_ids,\s*int64_t n_rows,\s*const int64_t\* hist_ptr,"
                     r"\s*const int32_t\* hist_items,\s*const int64_t\* gt_ptr,\s*const int32_t\* "
                     r"gt_items,\s*int32_t n_neg,\s*uint64_t seed,\s*int32_t\* neg_count,"
                     r"\s*int32_t\* negatives\);", core)
    assert re.search(r"int frecsys_rank_candidates_metrics\(frecsys_ctx\* ctx,[^;]*cand_ptr,[^;]*"
                     r"k_list,\s*int32_t nk,\s*float\* recall,\s*float\* ndcg\);", core)
    assert re.search(r"int frecsys_sampled_metrics\(frecsys_ctx\* ctx,[^;]*int32_t n_neg,\s*"
                     r"uint64_t seed,[^;]*int32_t\* neg_count,\s*int32_t\* negatives\);", core)
    for name in MODEL:
        assert re.search(r"int %s\(frecsys_model\* m,[^;]*float\* summary\);" % name, model), name
    raw = open(os.path.join(ROOT, "include", "frecsys_hip.h")).read()
    assert "NOT estimates of the full-catalogue metrics" in re.sub(r"\s*\n \*\s*", " ", raw)
    assert set(CORE) <= _exported(fh.LIB_PATH) and set(CORE) <= set(fh.EXPORTS)
    assert set(MODEL) <= _exported(fh.MODEL_LIB_PATH) and set(MODEL) <= set(fh.MODEL_EXPORTS)
    assert callable(fh.sample_negatives)
    assert callable(fh.Context.rank_candidates_metrics) and callable(fh.Context.sampled_metrics)
    for name in ("evaluate_candidates", "evaluate_candidates_fold_in", "evaluate_sampled",
                 "evaluate_sampled_fold_in"):
        assert callable(getattr(fh.Model, name)), name
    lib, ml = fh.load_library(), fh.load_model_library()
    out = np.zeros(4, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    one = np.ones(1, np.int32)
    assert lib.frecsys_sampled_metrics(None, 0, None, 1, 0, None, None, None, 1, 0, P(one), 1,
                                       P(out), P(out), None, None) == fh.ERR_INVALID
    assert lib.frecsys_rank_candidates_metrics(None, 0, None, 1, None, None, 0, None, None, None,
                                               P(one), 1, P(out), P(out)) == fh.ERR_INVALID
    for name in MODEL:
        assert getattr(ml, name) is not None
