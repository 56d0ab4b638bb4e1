"""The float64 reference and the case plans of the nearest-neighbour tests
(tests/similar_ref.py), and the surface of the feature, checked without a GPU:
similar64 on hand-made tables, the values the plans cover, the header
declarations, the exported symbols, the Python names and the C entry points'
null-handle answer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import recommend_ref as RR
import similar_ref as SR
from conftest import ROOT

fh = pytest.importorskip("frecsys_hip")


def test_similar64_hand_made():
    # rows 0 and 3 equal in value, row 2 zero, row 1 opposite to row 0
    T = np.array([[1, 0], [-2, 0], [0, 0], [1, 0], [3, 4]], np.float32)
    S, ids, sc = SR.similar64(T, [0, 2, 0], 3, True, False, None)
    assert ids.tolist() == [[3, 4, 2], [0, 1, 3], [3, 4, 2]]      # self excluded, ties by id
    np.testing.assert_allclose(sc, [[1.0, 0.6, 0.0], [0, 0, 0], [1.0, 0.6, 0.0]], atol=1e-15)
    assert not np.signbit(sc).any() and S[0, 0] == -np.inf and S[1, 2] == -np.inf
    _, ids, sc = SR.similar64(T, [0, 2], 3, True, True, None)
    assert ids.tolist() == [[0, 3, 4], [0, 1, 2]]                 # self kept; the zero row too
    assert sc[0, 0] == sc[0, 1] == 1.0 and (sc[1] == 0).all()
    _, ids, sc = SR.similar64(T, None, 2, False, False, None)     # dot: the large row wins
    assert ids[:, 0].tolist() == [4, 2, 0, 4, 0] and sc[0].tolist() == [3.0, 1.0]
    assert ids[2].tolist() == [0, 1] and ids[1].tolist() == [2, 0]   # -0.0 ties +0.0, by id
    # k above the eligible count, then an all-zero mask
    mask = np.array([1, 0, 1, 1, 0], np.uint8)
    _, ids, sc = SR.similar64(T, [3, 1], 7, True, False, mask)
    assert ids.tolist() == [[0, 2, -1, -1, -1, -1, -1], [2, 0, 3, -1, -1, -1, -1]]
    assert np.isneginf(sc[0, 2:]).all() and sc[1, :3].tolist() == [0.0, -1.0, -1.0]
    _, ids, sc = SR.similar64(T, None, 2, True, True, np.zeros(5, np.uint8))
    assert (ids == -1).all() and np.isneginf(sc).all()


def test_plans_cover_every_value():
    main = SR.dot_main()
    assert {(p[0], p[3]) for p in main} == {(m, d) for m in SR.GRID_M for d in SR.GRID_DIMS}
    for idx, want in ((1, SR.GRID_ROWS), (2, SR.GRID_KINDS), (4, ("none", "m70")),
                      (5, (False, True)), (6, (SR.USER, SR.ITEM)), (7, (None, 1))):
        assert {p[idx] for p in main} == set(want), idx
        for m in SR.GRID_M[2:]:   # and with every table size of more than one tile row
            if idx in (1, 2):
                assert len({p[idx] for p in main if p[0] == m}) >= 3, (idx, m)
            else:
                assert {p[idx] for p in main if p[0] == m} == set(want), (idx, m)
    plan = SR.dot_plan()
    singles = plan[len(main):]
    assert any(p[4] == "zero" for p in singles) and any(p[2] > p[0] for p in singles)
    # eligible counts at the buffer edges, self kept (m) and excluded (m - 1)
    edge = {(p[0] - (0 if p[5] else 1), p[2], p[5]) for p in singles if p[1] == 5}
    assert edge == {(m, k, keep) for m, k in RR.CAP_EDGE for keep in (False, True)}
    assert {511, 512, 513, 2047, 2048, 2049} == {e[0] for e in edge}
    assert {33, 200, 1024} <= {p[2] for p in singles if p[0] == 5000 and p[7] == 1}
    cos = SR.cosine_plan()
    assert {p[0] for p in cos} == set(SR.GRID_M) and {p[3] for p in cos} == set(SR.GRID_DIMS)
    assert {p[1] for p in cos} == set(SR.GRID_ROWS) and {1, 33, 1024} <= {p[2] for p in cos}
    assert {p[5] for p in cos} == {False, True} and {p[8] for p in cos} == {False, True}
    assert {p[6] for p in cos} == {SR.USER, SR.ITEM} and {p[7] for p in cos} == {None, 1}
    gauss = SR.gauss_plan()
    assert {(p[0], p[3]) for p in gauss} == {(m, d) for m in SR.GAUSS_M for d in SR.GAUSS_DIMS}
    assert {p[2] for p in gauss} == set(SR.GAUSS_KS)
    assert {p[5] for p in gauss} == {False, True} and {p[4] for p in gauss} == {"none", "m70"}
    assert {p[6] for p in gauss} == {SR.USER, SR.ITEM}


def test_query_rows_hold_the_seams():
    for m in SR.GRID_M:
        for n in SR.GRID_ROWS:
            rows = SR.query_rows(m, n, 1)
            assert len(rows) == n and rows.min() >= 0 and rows.max() < m
            if n >= 63:
                assert {r for r in (0, 127, 128, m - 1) if r < m} <= set(rows.tolist())
                assert len(set(rows.tolist())) < n    # a repeated id
    assert SR.query_rows(5000, 1, 1).tolist() == [4999]


def test_inputs_are_what_the_exact_tests_need():
    T = SR.grid_table(257, 64, 5)
    assert set(np.unique(T).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    np.testing.assert_array_equal(T, RR.grid_inputs(257, 3, 1, 64, 5)[1])
    Z = SR.sign_table(129, 200, 6, True)
    assert not Z[0].any() and not Z[128].any() and (np.abs(Z[1:128]) == 1).all()
    G = SR.gauss_table(1025, 20, 7)
    nrm = np.linalg.norm(G.astype(np.float64), axis=1)
    assert nrm.max() / nrm.min() > 300    # close to three decades
    rows = SR.query_rows(1025, 65, 7)
    _, by_cos, _ = SR.similar64(G, rows, 10, True, False, None)
    _, by_dot, _ = SR.similar64(G, rows, 10, False, False, None)
    assert (by_cos != by_dot).mean() > 0.5
    assert SR.cosine_tol(256) == 520 * 2.0 ** -24


def _declared(path):
    txt = open(os.path.join(ROOT, "include", path)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_headers_declare_the_entry_points():
    raw = open(os.path.join(ROOT, "include", "frecsys_hip.h")).read()
    assert re.search(r"#define FRECSYS_SIM_COSINE\s+1\b", raw)
    assert re.search(r"#define FRECSYS_SIM_KEEP_SELF\s+2\b", raw)
    core, model = _declared("frecsys_hip.h"), _declared("frecsys_model.h")
    assert re.search(r"int frecsys_similar\(frecsys_ctx\* ctx,\s*int32_t side,\s*const int64_t\* rows,"
                     r"\s*int64_t n_rows,\s*int32_t k,\s*int32_t flags,\s*const uint8_t\* mask,"
                     r"\s*int32_t\* ids,\s*float\* scores\);", core)
    for name, arg in (("frecsys_model_similar_items", "items"),
                      ("frecsys_model_similar_users", "users")):
        assert re.search(r"int %s\(frecsys_model\* m,\s*const int64_t\* %s,\s*int64_t n,\s*"
                         r"int32_t k,\s*int32_t flags,[^;]*int32_t\* ids,\s*float\* scores\);"
                         % (name, arg), model), name


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r" T (frecsys_\w+)", out))


def test_libraries_export_and_python_names():
    assert "frecsys_similar" in _exported(fh.LIB_PATH)
    assert {"frecsys_model_similar_items", "frecsys_model_similar_users"} <= _exported(
        fh.MODEL_LIB_PATH)
    assert "frecsys_similar" in fh.EXPORTS
    assert {"frecsys_model_similar_items", "frecsys_model_similar_users"} <= set(fh.MODEL_EXPORTS)
    assert (fh.SIM_COSINE, fh.SIM_KEEP_SELF) == (1, 2)
    assert callable(fh.Context.similar)
    assert callable(fh.Model.similar_items) and callable(fh.Model.similar_users)
    assert fh.load_library().frecsys_similar is not None
    ml = fh.load_model_library()
    assert ml.frecsys_model_similar_items is not None and ml.frecsys_model_similar_users is not None


def test_entry_points_reject_a_null_handle():
    lib = fh.load_library()
    ids = np.zeros(4, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.frecsys_similar(None, fh.SIDE_ITEM, None, 1, 2, fh.SIM_COSINE, None, P(ids),
                               None) == fh.ERR_INVALID
    ml = fh.load_model_library()
    assert ml.frecsys_model_similar_items(None, None, 1, 2, 0, None, P(ids), None) == fh.ERR_INVALID
    assert ml.frecsys_model_similar_users(None, None, 1, 2, 0, None, P(ids), None) == fh.ERR_INVALID
