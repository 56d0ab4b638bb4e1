"""The list-quality definitions on the host (frecsys_list_quality,
frecsys_exposure_summary; no GPU): against the pairwise float64 reference of
tests/quality_ref.py within the derived bound, exposure and its summary
exactly, every argument fault, and header / exports / ctypes consistency."""
import ctypes
import os
import re

import numpy as np
import pytest

import quality_ref as Q
from conftest import ROOT

fh = pytest.importorskip("frecsys_hip")


def _check(T, L, ks, w):
    ild, nov, ex = fh.list_quality(T, L, ks, w)
    r_ild, r_nov, r_ex = Q.quality64(T, L, ks, w)
    e_ild = Q.close(ild, r_ild)
    e_nov = Q.close(nov, r_nov) if w is not None else 0.0
    print(f"dim {T.shape[1]} k_list {tuple(ks)}: ild {e_ild:.3f} novelty {e_nov:.3f} of the bound")
    assert e_ild <= 1.0 and e_nov <= 1.0
    assert ild.dtype == np.float32 and ex.dtype == np.int64
    np.testing.assert_array_equal(ex, r_ex)
    assert (nov is None) == (w is None)
    return ild, nov, ex


@pytest.mark.parametrize("dim", Q.DIMS)
def test_list_quality_matches_reference(dim):
    T = Q.item_table(Q.M, dim, 9100 + dim)
    L = Q.caller_lists(Q.M, Q.M, 9200 + dim)
    w = Q.item_weights(Q.M, 9300 + dim)
    ild, nov, _ = _check(T, L, Q.K300, w)
    _check(T, L, Q.K_UNSORTED, None)
    # the same cut-off gives the same bytes wherever it stands in k_list
    u_ild, u_nov, _ = fh.list_quality(T, L, Q.K_UNSORTED, w)
    for q, K in enumerate(Q.K_UNSORTED):
        np.testing.assert_array_equal(u_ild[:, q].view(np.uint32),
                                      ild[:, Q.K300.index(K)].view(np.uint32))
        np.testing.assert_array_equal(u_nov[:, q].view(np.uint32),
                                      nov[:, Q.K300.index(K)].view(np.uint32))
    # the named rows: nothing filled, one slot, one item repeated, zero rows only
    assert (ild[0] == 0).all() and (nov[0] == 0).all()
    assert (ild[1] == 0).all() and (nov[1, :2] == 0).all() and (nov[1, 2:] == w[5]).all()
    assert ild[3, 0] == 0 and (np.abs(ild[3, 1:]) <= Q.BOUND).all()
    assert (nov[3] == w[33]).all()
    assert ild[8, 0] == 0 and (ild[8, 1:] == 1).all()


def test_k_limit_and_strided_table():
    T = Q.item_table(Q.M_BIG, Q.DIM_BIG, 9400)
    L = Q.caller_lists(Q.M_BIG, 1024, 9401, rows=10)
    w = Q.item_weights(Q.M_BIG, 9402)
    ild, nov, ex = _check(T, L, Q.K_BIG, w)
    wide = np.zeros((Q.M_BIG, Q.DIM_BIG + 5), np.float32)
    wide[:, :Q.DIM_BIG] = T
    got = fh.list_quality(wide[:, :Q.DIM_BIG], L, Q.K_BIG, w)   # ld = dim + 5
    for a, b in zip(got, (ild, nov, ex)):
        np.testing.assert_array_equal(a, b)


def test_exposure_summary_is_exact():
    rng = np.random.default_rng(9500)
    cases = [
        (np.zeros(50, np.int64), None),                                  # nothing exposed
        (np.eye(1, 50, 17, dtype=np.int64)[0] * 12345, None),            # one item holds everything
        (np.full(50, 7, np.int64), None),                                # uniform
        (rng.integers(0, 1000, 300), None),
        (rng.integers(0, 1000, 300), rng.random(300) < 0.3),             # a masked catalogue
        (rng.integers(0, 5, 300), np.zeros(300, bool)),                  # nothing eligible
        (rng.integers(0, 2 ** 40, 64), None),                            # a numerator beyond 2^53
    ]
    for counts, mask in cases:
        got = fh.exposure_summary(counts, mask)
        want = Q.summary_exact(counts, mask)
        if max(counts) < 2 ** 32:   # numerator and M S below 2^53: one rounding on either side
            assert got == want, (got, want)
        else:
            assert got["total"] == want["total"] and got["covered"] == want["covered"]
            assert abs(got["gini"] - want["gini"]) <= 2.0 ** -51
    one = fh.exposure_summary(cases[1][0])
    assert one["coverage"] == 1 / 50 and one["gini"] == 49 / 50
    assert fh.exposure_summary(cases[2][0]) == {"coverage": 1.0, "gini": 0.0, "total": 350,
                                                "covered": 50}
    assert fh.exposure_summary(cases[0][0]) == {"coverage": 0.0, "gini": 0.0, "total": 0,
                                                "covered": 0}


def test_summary_of_list_quality_exposure():
    T = Q.item_table(Q.M, 16, 9600)
    L = Q.caller_lists(Q.M, Q.M, 9601)
    ex = fh.list_quality(T, L, Q.K300)[2]
    mask = np.random.default_rng(9602).random(Q.M) < 0.5
    for q in range(len(Q.K300)):
        assert fh.exposure_summary(ex[q]) == Q.summary_exact(ex[q])
        assert fh.exposure_summary(ex[q], mask) == Q.summary_exact(ex[q], mask)


def test_argument_faults():
    lib, P = fh.load_library(), fh._ptr
    T = Q.item_table(Q.M, 8, 9700)
    L = np.zeros((3, 10), np.int32)
    w = np.ones(Q.M, np.float32)
    ild, nov = np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32)
    ex = np.ones((2, Q.M), np.int64)

    def call(table=T, lists=L, n=3, list_k=10, ks=(1, 10), nk=None, weight=w, o_ild=ild,
             o_nov=nov, o_ex=ex, n_items=Q.M, dim=8, ld=8):
        k = None if ks is None else np.asarray(ks, np.int32)
        rc = lib.frecsys_list_quality(P(table), n_items, dim, ld, P(lists), n, list_k, P(k),
                                      len(ks) if nk is None else nk, P(weight), P(o_ild), P(o_nov),
                                      P(o_ex))
        return rc, lib.frecsys_last_error(None).decode()

    assert call()[0] == fh.OK
    bad_w = w.copy()
    bad_w[4] = np.inf
    big = L.copy()
    big[2, 9] = Q.M
    faults = [
        (dict(ks=(0, 10)), "list_quality: cut-offs must be in [1, 10]"),
        (dict(ks=(1, 11)), "list_quality: cut-offs must be in [1, 10]"),
        (dict(ks=(1, 1025), list_k=2000, lists=np.zeros((3, 2000), np.int32)),
         "list_quality: cut-offs must be in [1, 1024]"),
        (dict(ks=None, nk=2), "list_quality: k_list must hold 1 to 32 cut-offs"),
        (dict(nk=0), "list_quality: k_list must hold 1 to 32 cut-offs"),
        (dict(ks=(1,) * 33), "list_quality: k_list must hold 1 to 32 cut-offs"),
        (dict(weight=None), "list_quality: novelty needs item_weight"),
        (dict(o_nov=None), "list_quality: item_weight without a novelty output"),
        (dict(weight=bad_w), "list_quality: item_weight[4] is not finite"),
        (dict(weight=None, o_ild=None, o_nov=None, o_ex=None),
         "list_quality: every output is null"),
        (dict(lists=big), f"list_quality: item id {Q.M} out of range"),
        (dict(n=-1), "list_quality: negative row count"),
        (dict(lists=None), "list_quality: null lists"),
        (dict(n=2 ** 62), "list_quality: n * list_k overflows"),
        (dict(table=None), "list_quality: bad item table (null, dim < 1, ld < dim)"),
        (dict(ld=7), "list_quality: bad item table (null, dim < 1, ld < dim)"),
        (dict(list_k=0), "list_quality: list_k must be positive"),
        (dict(n_items=0), "list_quality: n_items must be positive"),
    ]
    for kw, msg in faults:
        ex[:] = 1
        rc, err = call(**kw)
        assert (rc, err) == (fh.ERR_INVALID, msg), (kw.keys(), rc, err)
        assert (ex == 1).all()                       # nothing written
    # exposure alone needs no table; zero rows zero a given exposure array
    assert call(table=None, weight=None, o_ild=None, o_nov=None)[0] == fh.OK
    assert ex.sum() == ex[:, 0].sum() == 3 + 30     # item 0: 3 slots below K = 1, 30 below K = 10
    ex[:] = 1
    assert call(n=0, lists=None)[0] == fh.OK and (ex == 0).all()
    assert lib.frecsys_exposure_summary(None, 5, None, None, None, None, None) == fh.ERR_INVALID
    neg = np.array([1, -1, 2], np.int64)
    assert lib.frecsys_exposure_summary(P(neg), 3, None, None, None, None, None) == fh.ERR_INVALID
    assert lib.frecsys_last_error(None).decode() == "exposure_summary: negative count"
    # the device entry points refuse a null context before anything else
    assert lib.frecsys_rank_quality(None, 0, None, 0, 0, None, None, 0, 0, 0.5, 0, None, None,
                                    None, None, None, None, None, None) == fh.ERR_INVALID
    assert lib.frecsys_lists_quality(None, None, 0, 1, None, 0, None, None, None,
                                     None) == fh.ERR_INVALID


CORE = {"frecsys_list_quality": 13, "frecsys_exposure_summary": 7, "frecsys_rank_quality": 19,
        "frecsys_lists_quality": 10}
MODEL = {"frecsys_model_evaluate_quality": 21, "frecsys_model_evaluate_quality_fold_in": 22,
         "frecsys_model_list_quality": 12}


def _params(header, name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", txt)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_header_exports_and_signatures_agree():
    lib, mlib = fh.load_library(), fh.load_model_library()
    for names, header, exports, l in ((CORE, "frecsys_hip.h", fh.EXPORTS, lib),
                                      (MODEL, "frecsys_model.h", fh.MODEL_EXPORTS, mlib)):
        for name, count in names.items():
            params = _params(header, name)
            fn = getattr(l, name)
            assert name in exports
            assert len(params) == count == len(fn.argtypes), (name, params)
            for p, t in zip(params, fn.argtypes):   # pointers, then the scalar widths
                want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float")
                        else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int32)
                assert t is want, (name, p, t)
    txt = open(os.path.join(ROOT, "include", "frecsys_hip.h")).read()
    for word in ("ILD@K", "Novelty@K", "Exposure.", "2^-23", "frecsys_list_quality: the definition"):
        assert word in txt, word
    for name in ("rank_quality", "lists_quality"):
        assert callable(getattr(fh.Context, name))
    for name in ("evaluate_quality", "evaluate_quality_fold_in", "list_quality",
                 "item_self_information"):
        assert callable(getattr(fh.Model, name))
    assert callable(fh.list_quality) and callable(fh.exposure_summary)
