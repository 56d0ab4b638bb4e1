"""frecsys_mmr_select, the host definition of the MMR calls, against the
float64 greedy of tests/diverse_ref.py; its properties; the names the feature
adds and the rejections that need no device.

test_exact_against_float64     sign tables x grid queries, raw scores: every
                               quantity an exact dyadic float32, so selections
                               and values equal float64's outright (600 rows).
test_normalised_gauss          Gaussian tables, normalised relevance: equal to
                               float64 on every step before a row's first
                               close call.
test_properties                lam = 1, k = p, empty slots, p < k, equal
                               scores, a zero row, twins, no -0.0.
test_names_exported            headers, libraries, EXPORTS, methods.
test_rejections                every FRECSYS_ERR_INVALID case, no device call.
"""
import os
import re

import numpy as np
import pytest

import diverse_ref as D
import frecsys_hip as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = D.FLT_MAX


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("dim", (16, 64, 256))
def test_exact_against_float64(dim):
    n, m, pool, k = 40, 300, 64, 24
    T, ids, scores = D.exact_case(dim, n, m, pool, 7100 + dim)
    rows = 0
    for lam in (0.0, 0.25, 0.5, 0.75, 1.0):
        items, sc, mmr = fh.mmr_select(T, ids, scores, k, lam, raw_scores=True, return_mmr=True)
        slots, vals, _ = D.mmr64(T, ids, scores, k, lam, True, 0.0)
        assert (slots >= 0).all()
        assert np.array_equal(items, np.take_along_axis(ids, slots, 1))
        assert np.array_equal(bits(sc), bits(np.take_along_axis(scores, slots, 1)))
        assert np.array_equal(mmr.astype(np.float64), vals)  # exact dyadic values
        mi, ms, mm = D.mmr32(T, ids, scores, k, lam, True)
        assert np.array_equal(items, mi) and np.array_equal(bits(sc), bits(ms))
        assert np.array_equal(bits(mmr), bits(mm))
        rows += n
    assert rows == 200  # x 3 dims = 600 rows


GAUSS = [(20, 600, 100, 20), (64, 2000, 200, 50)]


@pytest.mark.parametrize("dim,m,pool,k", GAUSS, ids=[f"d{c[0]}" for c in GAUSS])
@pytest.mark.parametrize("lam", (0.3, 0.7))
def test_normalised_gauss(dim, m, pool, k, lam):
    """tol = 1e-5: twice the worst-case float32 error of v at d <= 64, about
    (d + 3) 2^-24 for the cosine plus two roundings."""
    tol, n = 1e-5, 48
    T, ids, scores = D.gauss_case(dim, n, m, pool, 7200 + dim)
    items, sc, mmr = fh.mmr_select(T, ids, scores, k, lam, return_mmr=True)
    slots, vals, flag = D.mmr64(T, ids, scores, k, lam, False, tol)
    # from the reference alone: most steps lie before a row's first close call
    share = flag.sum() / (n * k)
    print(f"d={dim} lam={lam}: {share:.3f} of the steps compared")
    assert share >= 0.8
    want = np.take_along_axis(ids, slots, 1)
    worst = 0.0
    for i in range(n):
        t = int(flag[i])
        assert np.array_equal(items[i, :t], want[i, :t]), i
        if t:
            worst = max(worst, float(np.abs(mmr[i, :t] - vals[i, :t]).max()))
    print(f"worst mmr error {worst:.2e}")
    assert worst <= tol


def test_properties():
    rng = np.random.default_rng(7300)
    m, dim, pool = 200, 24, 40
    T = D.gauss_table(m, dim, 7301)
    X = rng.standard_normal((12, dim)).astype(np.float32)
    ids, scores = D.top_pools(X, T, pool)
    # lam = 1: the first k of the pool in (score, slot) order, in both modes
    for raw in (False, True):
        items, sc, mmr = fh.mmr_select(T, ids, scores, 15, 1.0, raw_scores=raw, return_mmr=True)
        assert np.array_equal(items, ids[:, :15]) and np.array_equal(bits(sc), bits(scores[:, :15]))
        if raw:
            assert np.array_equal(bits(mmr), bits(scores[:, :15] + np.float32(0.0)))
    # ... also when the pool is not sorted: by score, ties by slot
    sh = np.array([[3, 7, 9, 7, 1, 9]], np.int32)
    ss = np.array([[1.0, 2.0, 0.5, 2.0, -1.0, 0.5]], np.float32)
    items, sc = fh.mmr_select(T, sh, ss, 6, 1.0)
    assert items.tolist() == [[7, 7, 3, 9, 9, 1]] and sc.tolist() == [[2.0, 2.0, 1.0, 0.5, 0.5, -1.0]]
    # k = p: a permutation of the filled slots
    items, sc = fh.mmr_select(T, ids, scores, pool, 0.4)
    assert np.array_equal(np.sort(items, 1), np.sort(ids, 1))
    assert np.array_equal(np.sort(sc, 1), np.sort(scores, 1))
    # empty slots in the middle and at the tail; p < k pads
    holes = ids.copy()
    holes[:, 5:12] = -1
    holes[:, 30:] = -1
    p = 40 - 7 - 10
    items, sc, mmr = fh.mmr_select(T, holes, scores, 30, 0.6, return_mmr=True)
    assert (items[:, :p] >= 0).all() and (items[:, p:] == -1).all()
    assert (sc[:, p:] == -FLT_MAX).all() and (mmr[:, p:] == -FLT_MAX).all()
    assert np.array_equal(np.sort(items[:, :p], 1), np.sort(holes[holes >= 0].reshape(12, p), 1))
    mi, ms, mm = D.mmr32(T.astype(np.float32), holes, scores, 30, 1.0, True)
    assert np.array_equal(fh.mmr_select(T, holes, scores, 30, 1.0, raw_scores=True)[0], mi)
    none = np.full((2, 5), -1, np.int32)
    items, sc, mmr = fh.mmr_select(T, none, np.zeros((2, 5), np.float32), 3, 0.5, return_mmr=True)
    assert (items == -1).all() and (sc == -FLT_MAX).all() and (mmr == -FLT_MAX).all()
    # all scores equal: rel = 0, the first pick is slot 0 at value +0
    flat = np.full_like(scores, 2.5)
    items, sc, mmr = fh.mmr_select(T, ids, flat, 4, 0.5, return_mmr=True)
    assert np.array_equal(items[:, 0], ids[:, 0]) and (bits(mmr[:, 0]) == 0).all()
    # a zero item row: inv = 0, cosine +0 with everything
    Z = T.copy()
    Z[7] = 0.0
    zi = np.array([[7, 1, 2]], np.int32)
    zs = np.array([[3.0, 2.0, 1.0]], np.float32)
    items, sc, mmr = fh.mmr_select(Z, zi, zs, 3, 0.5, raw_scores=True, return_mmr=True)
    assert items[0, 0] == 7 and mmr[0, 0] == 1.5
    c12 = float(Z[1].astype(np.float64) @ Z[2] / np.linalg.norm(Z[1]) / np.linalg.norm(Z[2]))
    assert items[0, 1] == 1 and mmr[0, 1] == 1.0  # 0.5 * 2 - 0.5 * (+0)
    assert abs(mmr[0, 2] - (0.5 - 0.5 * max(0.0, c12))) < 1e-6
    # twins: the copy of an item row is selected last at lam < 1
    W = T.copy()
    W[11] = W[10]
    tw = np.array([[10, 11, 20, 21, 22, 23]], np.int32)
    ts = np.array([[5.0, 5.0, 1.0, 0.9, 0.8, 0.7]], np.float32)
    items, _ = fh.mmr_select(W, tw, ts, 6, 0.3)
    assert items[0, 0] == 10 and items[0, 5] == 11
    # no -0.0: at lam = 0 a negative raw score gives base = 0 * score = -0.0, and
    # behind a zero row (cosine +0) base - oml * m = -0.0 - 0.0 = -0.0; the
    # + 0.0f of every value turns both into +0
    items, sc, mmr = fh.mmr_select(Z, np.array([[7, 1, 2]], np.int32),
                                   np.array([[-2.0, -3.0, -1.0]], np.float32), 3, 0.0,
                                   raw_scores=True, return_mmr=True)
    assert np.float32(0.0) * np.float32(-2.0) == 0 and bits(np.float32(0.0) * np.float32(-2.0)) != 0
    assert bits(mmr)[0, 0] == 0 and bits(mmr)[0, 1] == 0  # step 0, and step 1 behind the zero row
    assert items.tolist()[0][:2] == [7, 1]


def test_names_exported():
    def decls(path):
        txt = open(os.path.join(ROOT, "include", path)).read()
        return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    core, model = decls("frecsys_hip.h"), decls("frecsys_model.h")
    assert re.search(r"int frecsys_recommend_diverse\(frecsys_ctx\* ctx, int32_t side,[^;]*"
                     r"int32_t k, int32_t pool, float lam, int32_t flags,[^;]*float\* mmr\);", core)
    assert re.search(r"int frecsys_diversify\(frecsys_ctx\* ctx, const int32_t\* lists,[^;]*"
                     r"int32_t pool, int32_t k, float lam, int32_t flags,[^;]*float\* mmr\);", core)
    assert re.search(r"int frecsys_mmr_select\(const float\* item_table, int64_t n_items, "
                     r"int32_t dim, int64_t ld,[^;]*float\*\s*mmr\);", core)
    assert re.search(r"#define FRECSYS_DIV_RAW_SCORES 2", core)
    core_names = {"frecsys_recommend_diverse", "frecsys_diversify", "frecsys_mmr_select"}
    model_names = {"frecsys_model_recommend_diverse", "frecsys_model_recommend_diverse_fold_in",
                   "frecsys_model_diversify"}
    for name in model_names:
        assert re.search(r"int %s\(frecsys_model\* m,[^;]*float\* mmr\);" % name, model), name
    assert core_names <= set(fh.EXPORTS) and model_names <= set(fh.MODEL_EXPORTS)
    lib, ml = fh.load_library(), fh.load_model_library()
    for name in core_names:
        assert getattr(lib, name) is not None
    for name in model_names:
        assert getattr(ml, name) is not None
    assert fh.DIV_RAW_SCORES == 2
    assert callable(fh.mmr_select)
    assert callable(fh.Context.recommend_diverse) and callable(fh.Context.diversify)
    for name in ("recommend_diverse", "recommend_diverse_fold_in", "diversify"):
        assert callable(getattr(fh.Model, name))
    assert [fh.default_pool(k) for k in (1, 20, 256, 300, 1024)] == [4, 80, 1024, 1024, 1024]


def test_rejections():
    lib = fh.load_library()
    T = np.ones((10, 4), np.float32)
    ids = np.zeros((2, 8), np.int32)
    sc = np.zeros((2, 8), np.float32)
    items = np.zeros((2, 8), np.int32)
    out = np.zeros((2, 8), np.float32)
    P = fh._ptr

    def select(k=3, pool=8, lam=0.5, flags=0, n=2, tab=T, n_items=10, dim=4, ld=4, lists=ids,
               scores=sc, o_items=items, o_scores=out):
        return lib.frecsys_mmr_select(P(tab), n_items, dim, ld, P(lists), P(scores), n, pool, k, lam,
                                      flags, P(o_items), P(o_scores), None)

    assert select() == fh.OK
    bad = [dict(k=0), dict(k=9), dict(pool=0), dict(pool=1025, k=1), dict(lam=-0.01),
           dict(lam=1.01), dict(lam=float("nan")), dict(flags=1), dict(flags=4), dict(n=-1),
           dict(o_items=None), dict(o_scores=None), dict(tab=None), dict(lists=None),
           dict(scores=None), dict(n_items=0), dict(dim=0), dict(ld=3)]
    for kw in bad:
        assert select(**kw) == fh.ERR_INVALID, kw
    for kw in bad:  # zero rows are fine only with sound arguments
        if "n" not in kw and not ({"o_items", "o_scores", "tab", "lists", "scores", "n_items",
                                   "dim", "ld"} & set(kw)):
            assert select(n=0, **kw) == fh.ERR_INVALID, kw
    assert select(n=0, o_items=None, o_scores=None, lists=None, scores=None) == fh.OK
    big = ids.copy()
    big[1, 3] = 10
    assert select(lists=big) == fh.ERR_INVALID
    for v in (np.inf, -np.inf, np.nan):
        s2 = sc.copy()
        s2[0, 2] = v
        assert select(scores=s2) == fh.ERR_INVALID
        e2 = ids.copy()
        e2[0, 2] = -1  # ... but not in an empty slot
        assert select(scores=s2, lists=e2) == fh.OK
    s3 = sc.copy()
    s3[0, 0], s3[0, 1] = FLT_MAX, -FLT_MAX
    assert select(scores=s3) == fh.ERR_INVALID  # the range overflows
    assert select(scores=s3, flags=fh.DIV_RAW_SCORES) == fh.OK
    # the device calls reject a null context before anything else
    assert lib.frecsys_diversify(None, P(ids), P(sc), 2, 8, 3, 0.5, 0, P(items), P(out),
                                 None) == fh.ERR_INVALID
    assert lib.frecsys_recommend_diverse(None, 0, None, 2, 3, 8, 0.5, 0, None, P(items), P(out),
                                         None) == fh.ERR_INVALID
    with pytest.raises(fh.FrecsysError):
        fh.mmr_select(T, ids, sc, 9)
