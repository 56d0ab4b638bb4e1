"""The surface of frecsys_audience and its host-only planner, checked without a
GPU: the header declarations, the exported symbols, the Python names, the C
entry points' null-handle answer, the invariants of frecsys_audience_plan over
a grid of shapes and knobs, the cover of the exact tests' plan and the float64
reference of tests/audience_ref.py against a brute-force loop."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import audience_ref as AR
from conftest import ROOT

fh = pytest.importorskip("frecsys_hip")

KNOBS = ("FRECSYS_AUDIENCE_THIN_MAX", "FRECSYS_RECOMMEND_SPLITS", "FRECSYS_RECOMMEND_WS_MB")
MERGE_WORDS = 8192      # what the last merge sorts in LDS (frecsys_hip.h)


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    """No knob of the caller's; the thin-query limit pinned (its default is a
    measured number: test_default_limit)."""
    for kn in KNOBS:
        monkeypatch.delenv(kn, raising=False)
    monkeypatch.setenv(KNOBS[0], "64")


def _declared(path):
    txt = open(os.path.join(ROOT, "include", path)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_headers_declare_the_entry_points():
    raw = open(os.path.join(ROOT, "include", "frecsys_hip.h")).read()
    assert re.search(r"#define FRECSYS_AUD_EXCLUDE_HISTORY\s+1\b", raw)
    core, model = _declared("frecsys_hip.h"), _declared("frecsys_model.h")
    assert re.search(r"int frecsys_audience\(frecsys_ctx\* ctx,\s*const int64_t\* items,\s*int64_t n,"
                     r"\s*int32_t k,\s*int32_t flags,\s*const uint8_t\* user_mask,"
                     r"\s*int32_t\* users,\s*float\* scores\);", core)
    assert re.search(r"typedef struct \{\s*int32_t thin, queries_per_pass, passes, splits, "
                     r"chunk_rows, slots,\s*merge_rounds;\s*int64_t rows_per_batch, "
                     r"workspace_bytes;\s*\} frecsys_audience_plan_t;", core)
    assert re.search(r"int frecsys_audience_plan\(int32_t dim,\s*int64_t n_users,\s*int64_t n,"
                     r"\s*int32_t k,\s*int32_t cus,\s*int32_t exclude,"
                     r"\s*frecsys_audience_plan_t\* out\);", core)
    assert re.search(r"int frecsys_model_audience\(frecsys_model\* m,\s*const int64_t\* items,"
                     r"\s*int64_t n,\s*int32_t k,\s*int32_t exclude_seen,"
                     r"\s*const uint8_t\* user_mask,\s*int32_t\* users,\s*float\* scores\);", model)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r" T (frecsys_\w+)", out))


def test_libraries_export_and_python_names():
    assert {"frecsys_audience", "frecsys_audience_plan"} <= _exported(fh.LIB_PATH)
    assert "frecsys_model_audience" in _exported(fh.MODEL_LIB_PATH)
    assert {"frecsys_audience", "frecsys_audience_plan"} <= set(fh.EXPORTS)
    assert "frecsys_model_audience" in fh.MODEL_EXPORTS
    assert fh.AUD_EXCLUDE_HISTORY == 1
    assert callable(fh.Context.audience) and callable(fh.Model.audience)
    assert callable(fh.audience_plan)
    assert fh.load_library().frecsys_audience is not None
    assert fh.load_model_library().frecsys_model_audience is not None


def test_entry_points_reject_a_null_handle():
    lib = fh.load_library()
    ids = np.zeros(4, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.frecsys_audience(None, None, 1, 2, 0, None, P(ids), None) == fh.ERR_INVALID
    ml = fh.load_model_library()
    assert ml.frecsys_model_audience(None, None, 1, 2, 0, None, P(ids), None) == fh.ERR_INVALID
    assert ml.frecsys_model_audience(None, None, 0, 2, 1, None, None, None) == fh.ERR_INVALID


PLAN_DIMS = (5, 64, 256, 1000)
PLAN_M = (1, 127, 128, 129, 5000, 116677, 2000000)
PLAN_N = (1, 7, 8, 9, 64, 65, 1024)
PLAN_K = (1, 33, 100, 128, 129, 1000, 1024)
PLAN_CUS = (1, 104, 256)


def _check_plan(p, dim, m, n, k, budget, thin_max):
    C, splits, qpp = p["chunk_rows"], p["splits"], p["queries_per_pass"]
    chunks = -(-m // C)
    # the splits tile [0, m) contiguously, in whole chunks, none of them empty
    assert 1 <= splits <= chunks
    edges = [s * chunks // splits for s in range(splits + 1)]
    assert edges[0] == 0 and edges[-1] == chunks and all(b > a for a, b in zip(edges, edges[1:]))
    assert edges[-1] * C >= m > (edges[-1] - 1) * C
    # a chunk always fits behind k kept candidates
    assert p["slots"] >= k + C and p["slots"] & (p["slots"] - 1) == 0
    assert p["thin"] == (1 if n <= thin_max else 0)
    assert 1 <= p["rows_per_batch"] <= n
    assert 1 <= qpp <= (8 if p["thin"] else 64)
    assert p["passes"] == -(-n // qpp)
    if p["rows_per_batch"] >= (8 if p["thin"] else 64):
        assert qpp == (8 if p["thin"] else 64)
    # the rounds (frecsys_hip.h): on the thin path every one but the last takes
    # the k best of groups of 8192 / kp lists of at most min(k, rows) words,
    # and the last has one list left to write out; the scan's merge sorts its
    # splits' words in LDS
    kp = 64
    while kp < k:
        kp *= 2
    lists, group = splits, MERGE_WORDS // kp
    assert p["merge_rounds"] >= 1 and group >= 2
    for _ in range(p["merge_rounds"] - 1):
        assert lists > 1                    # no round without need
        lists = -(-lists // group)
    assert lists * min(k, m) <= lists * k <= MERGE_WORDS
    assert lists == 1 or not p["thin"]
    if not p["thin"]:
        assert p["merge_rounds"] == 1 and C == 128
    # the batch regions: at least the lists and the outputs, within the budget
    assert p["workspace_bytes"] >= p["rows_per_batch"] * (splits * p["slots"] * 8 + k * 8)
    assert p["workspace_bytes"] <= budget


def test_plan_invariants():
    for dim, m, n, k, cus in itertools.product(PLAN_DIMS, PLAN_M, PLAN_N, PLAN_K, PLAN_CUS):
        for exclude in (False, True):
            p = fh.audience_plan(dim, m, n, k, cus=cus, exclude=exclude)
            _check_plan(p, dim, m, n, k, 256 << 20, 64)
    # the thin path's grid is not capped by the merge: every CU has work at any k
    for k in (100, 1000):
        p = fh.audience_plan(256, 116677, 1, k)
        assert p["thin"] == 1 and p["splits"] >= 256 and p["splits"] * k > MERGE_WORDS
        assert p["merge_rounds"] >= 3
        q = fh.audience_plan(256, 116677, 65, k)
        assert q["thin"] == 0 and q["splits"] * k <= MERGE_WORDS
    # the history bits are a part of the batch
    a = fh.audience_plan(64, 5000, 8, 33, exclude=False)
    b = fh.audience_plan(64, 5000, 8, 33, exclude=True)
    assert b["workspace_bytes"] - a["workspace_bytes"] == 8 * 4 * 4 * -(-5000 // 128)


def test_plan_follows_the_knobs(monkeypatch):
    shapes = [(64, 5000, n, k) for n in (1, 8, 17, 64, 65, 600) for k in (33, 100, 1024)]
    shapes += [(256, 116677, n, 100) for n in (1, 8, 64, 1024)]
    for thin_max in (0, 1, 16, 100000):
        monkeypatch.setenv("FRECSYS_AUDIENCE_THIN_MAX", str(thin_max))
        for dim, m, n, k in shapes:
            p = fh.audience_plan(dim, m, n, k)
            assert p["thin"] == (1 if n <= thin_max else 0)     # 0 forces the scan
            _check_plan(p, dim, m, n, k, 256 << 20, thin_max)
    monkeypatch.setenv("FRECSYS_AUDIENCE_THIN_MAX", "64")
    for mb in (1, 8):
        monkeypatch.setenv("FRECSYS_RECOMMEND_WS_MB", str(mb))
        for dim, m, n, k in shapes:
            for exclude in (False, True):
                p = fh.audience_plan(dim, m, n, k, exclude=exclude)
                _check_plan(p, dim, m, n, k, mb << 20, 64)
    monkeypatch.delenv("FRECSYS_RECOMMEND_WS_MB")
    for want in (1, 3, 7, 100000):
        monkeypatch.setenv("FRECSYS_RECOMMEND_SPLITS", str(want))
        for dim, m, n, k in shapes:
            p = fh.audience_plan(dim, m, n, k)
            chunks = -(-m // p["chunk_rows"])
            cap = chunks if p["thin"] else min(chunks, 64, MERGE_WORDS // k)
            assert p["splits"] == min(want, cap)
            _check_plan(p, dim, m, n, k, 256 << 20, 64)


def test_default_limit(monkeypatch):
    """Unset, the limit is one number: thin up to it, the scan above, and a
    single query is always thin."""
    monkeypatch.delenv(KNOBS[0])
    thin = [fh.audience_plan(256, 116677, n, 100)["thin"] for n in (2 ** e for e in range(21))]
    assert thin[0] == 1 and thin == sorted(thin, reverse=True)


def test_plan_rejects_bad_arguments():
    lib = fh.load_library()
    out = ctypes.create_string_buffer(64)       # room for the 48-byte plan
    ok = (64, 5000, 8, 33, 256, 0)
    assert lib.frecsys_audience_plan(*ok, out) == fh.OK
    for pos, bad in ((0, 0), (0, 1025), (1, 0), (2, 0), (2, -1), (3, 0), (3, 1025), (4, 0),
                     (5, 2), (5, -1)):
        args = list(ok)
        args[pos] = bad
        assert lib.frecsys_audience_plan(*args, out) == fh.ERR_INVALID, (pos, bad)
    assert lib.frecsys_audience_plan(*ok, None) == fh.ERR_INVALID
    with pytest.raises(fh.FrecsysError):
        fh.audience_plan(64, 0, 1, 5)


def test_grid_plan_covers_every_pair():
    C, QT, ms, ns = AR.grid_sizes(fh.audience_plan)
    assert (C, QT) == (fh.audience_plan(1000, 1, 17, 1024)["chunk_rows"],
                       fh.audience_plan(5, 2000000, 3, 1)["queries_per_pass"])
    main = AR.grid_main(fh.audience_plan)
    values = [ms, ns, AR.GRID_KINDS, AR.GRID_DIMS, (False, True), AR.GRID_MASKS]
    for a, b in itertools.combinations(range(6), 2):
        seen = {(c[a], c[b]) for c in main}
        assert seen == set(itertools.product(values[a], values[b])), (a, b)
    plan = AR.grid_plan(fh.audience_plan)
    assert len(plan) == AR.GRID_CASES
    assert len({c[-1] for c in plan}) == len(plan)          # a seed of its own each
    for m, n, k, dim, exclude, mk, splits, seed in plan:
        assert 1 <= k <= 1024
        assert fh.audience_plan(dim, m, n, k, exclude=exclude)["thin"] == 1
    # the capacity edges: one split, every user eligible, slots - 1 | slots | slots + 1
    for k in (33, 1024):
        slots = fh.audience_plan(5, 5000, 5, k)["slots"]
        assert {c[0] for c in plan if c[6] == 1 and c[2] == k and c[5] == "none"} >= {
            slots - 1, slots, slots + 1}
    # buffers compacted more than once: a sweep of 5,000 users in one split
    assert sum(1 for c in plan if c[0] == 5000 and c[6] == 1) >= 3


def test_grid_case_holds_the_special_rows():
    V, U, iptr, icol, items = AR.grid_case(257, 9, 33, 20, 1)
    assert V.shape == (10, 20) and U.shape == (257, 20) and len(iptr) == 11
    assert set(np.unique(V)) | set(np.unique(U)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert items.tolist() == [0, 1, 2, 3, 1, 5, 6, 7, 8]
    assert not V[5].any() and not U[128].any()
    rows = [icol[iptr[r]:iptr[r + 1]] for r in range(4)]
    assert len(rows[0]) == 0 and rows[1].tolist() == [0, 256]
    assert len(set(rows[2].tolist())) < len(rows[2])
    assert len(set(rows[3].tolist())) == 257 - 33 + 1


def test_audience64_against_a_loop():
    rng = np.random.default_rng(11)
    nu, ni, dim, k = 7, 4, 3, 5
    U = rng.integers(-2, 3, (nu, dim)).astype(np.float32)
    V = rng.integers(-2, 3, (ni, dim)).astype(np.float32)
    V[2] = -0.0
    iptr = np.array([0, 0, 2, 5, 5], np.int64)
    icol = np.array([6, 0, 3, 3, 1], np.int32)
    mask = np.array([1, 1, 0, 1, 1, 1, 1], np.uint8)
    items = np.array([3, 1, 2, 1], np.int64)
    for exclude, mk in itertools.product((False, True), (None, mask)):
        S, ids, sc = AR.audience64(V, U, iptr, icol, items, k, exclude, mk)
        for q, it in enumerate(items):
            cand = []
            for u in range(nu):
                if mk is not None and not mk[u]:
                    continue
                if exclude and u in icol[iptr[it]:iptr[it + 1]].tolist():
                    continue
                s = sum(float(V[it, c]) * float(U[u, c]) for c in range(dim)) + 0.0
                cand.append((-s, u))
            cand.sort()
            want = [u for _, u in cand[:k]] + [-1] * (k - len(cand[:k]))
            assert ids[q].tolist() == want
            for j, (ns, u) in enumerate(cand[:k]):
                assert sc[q, j] == -ns and (sc[q, j] != 0 or not np.signbit(sc[q, j]))
            assert np.isneginf(sc[q, len(cand[:k]):]).all()
        np.testing.assert_array_equal(ids[1], ids[3])       # a repeated query: the same list
