"""frecsys_dpp_select, the host definition of the DPP calls, against the
float64 greedy of tests/dpp_ref.py, brute-force determinants and its exact
identities; the names the feature adds and the rejections that need no device.

test_exp2_accuracy             dpp_exp2 through gain[0] on a dense grid.
test_against_float64           slots equal float64's before a row's first close
                               step, gains within a measured tolerance.
test_greedy_step_is_argmax_det every selection maximises det(L[sel + b]).
test_logdet_invariant          sum log gain = slogdet(L[sel, sel]).
test_exact_identities          orthogonal tables, twins, a zero row, the rank
                               bound, the fill, gain = None.
test_names_exported            headers, libraries, EXPORTS, methods.
test_rejections                every FRECSYS_ERR_INVALID case, no device call.
"""
import os
import re

import numpy as np
import pytest

import dpp_ref as R
import frecsys_hip as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = R.FLT_MAX


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_exp2_accuracy():
    """k = 1, raw scores, theta = 1: gain[0] = dpp_exp2(score) * 1 + 0.  The bar
    is include/frecsys_hip.h's, 1e-6 relative on [-64, 64] (derived there from
    the remainder and the roundings); measured worst: 6.6e-8."""
    x = np.concatenate([np.linspace(-64.0, 64.0, 400001), np.arange(-64.0, 64.5, 0.5),
                        np.arange(-64.0, 64.0, 1.0) + 0.4999999, [-80.0, 80.0, 1e-30, -1e-30]])
    x = x.astype(np.float32)
    T = np.array([[1.0, 0.0]], np.float32)
    ids = np.zeros((len(x), 1), np.int32)
    _, sc, gain = fh.dpp_select(T, ids, x[:, None], 1, theta=1.0, raw_scores=True,
                                return_gain=True)
    assert np.array_equal(bits(sc[:, 0]), bits(x))
    want = np.exp2(np.clip(x.astype(np.float64), -64.0, 64.0))
    err = np.abs(gain[:, 0].astype(np.float64) / want - 1.0)
    print(f"worst relative error of dpp_exp2: {err.max():.2e}")
    assert err.max() <= 1e-6
    # integers are exact, and the clamp holds
    ints = np.arange(-64, 65)
    _, _, g = fh.dpp_select(T, np.zeros((len(ints), 1), np.int32),
                            ints.astype(np.float32)[:, None], 1, theta=1.0, raw_scores=True,
                            return_gain=True)
    assert np.array_equal(g[:, 0].astype(np.float64), np.exp2(ints.astype(np.float64)))


# (dim, items, pool, k, theta, raw): k <= min(d, p) in all.  (theta = 0 is not
# here: its step 0 is a tie of every slot, close by definition; the exact
# identities cover it.)
F64_CASES = [(8, 400, 40, 8, 4.0, False), (20, 600, 100, 20, 4.0, False),
             (20, 600, 100, 20, 1.0, False), (64, 2000, 200, 50, 2.0, False),
             (64, 2000, 120, 40, 0.25, True), (256, 3000, 200, 60, 8.0, False)]
F64_ROWS = 24
# measured over F64_CASES (see test_against_float64 / test_logdet_invariant)
WORST_GAIN_DEV = 3.8e-6
WORST_LOGDET_DEV = 1.2e-5


def _f64_case(c):
    dim, m, pool, k, theta, raw = c
    T, ids, scores = R.gauss_case(dim, F64_ROWS, m, pool, 7400 + dim + pool)
    if raw:
        scores = (scores / np.abs(scores).max(1, keepdims=True)).astype(np.float32)
    return T, ids, scores


def test_against_float64():
    """Slots equal dpp64's before each row's first close step (best within 1e-4
    of the runner-up, or a residual within 1 % of eps); gains within 8 x the
    worst relative deviation measured over these cases.  Measured worst:
    3.75e-6 (WORST_GAIN_DEV; the gain is a 1e-6-accurate w times a residual
    that loses digits as it shrinks toward eps).  At least 90 % of all
    positions must be compared: the reference alone decides that share
    (measured: 93.6 %)."""
    eps = 1e-3
    compared = total = 0
    worst = 0.0
    for c in F64_CASES:
        T, ids, scores = _f64_case(c)
        k, theta, raw = c[3], c[4], c[5]
        items, sc, gain = fh.dpp_select(T, ids, scores, k, theta, eps, raw_scores=raw,
                                        return_gain=True)
        slots, g64, flag = R.dpp64(T, ids, scores, k, theta, eps, raw)
        want = np.take_along_axis(ids, slots, 1)
        for i in range(F64_ROWS):
            t = int(flag[i])
            assert np.array_equal(items[i, :t], want[i, :t]), (c, i)
            assert np.array_equal(bits(sc[i, :t]), bits(scores[i, slots[i, :t]])), (c, i)
            live = g64[i, :t] > 0
            if live.any():
                dev = np.abs(gain[i, :t][live] / g64[i, :t][live] - 1.0).max()
                worst = max(worst, float(dev))
            assert (gain[i, :t][~live] == 0).all()
            compared += t
        total += F64_ROWS * k
    print(f"compared {compared} of {total} positions ({compared / total:.3f}); "
          f"worst relative gain deviation {worst:.2e}")
    assert compared >= 0.9 * total
    assert worst <= 8 * WORST_GAIN_DEV


def test_greedy_step_is_argmax_det():
    """pool <= 8, k <= 4: at every DPP step the selected slot maximises the
    float64 det(L[sel + b]) over the candidates (up to the 1e-4 margin inside
    which float32 may pick the other)."""
    rng = np.random.default_rng(7500)
    checked = 0
    for dim, pool, k, theta in ((8, 8, 4, 2.0), (5, 7, 4, 0.0), (12, 6, 3, 6.0), (3, 8, 4, 1.0)):
        T = R.gauss_table(60, dim, 7501 + dim)
        X = rng.standard_normal((20, dim)).astype(np.float32)
        ids, scores = R.top_pools(X, T, pool)
        items, _, gain = fh.dpp_select(T, ids, scores, k, theta, 1e-3, return_gain=True)
        for i in range(len(ids)):
            filled, L = R.kernel64(T, ids[i], scores[i], theta, False)
            sel = []
            for t in range(k):
                if gain[i, t] == 0:
                    break  # the fallback: pool order, not a determinant
                dets = np.array([np.linalg.det(L[np.ix_(sel + [b], sel + [b])])
                                 if b not in sel else -np.inf for b in range(len(filled))])
                s = int(np.flatnonzero(ids[i] == items[i, t])[0])
                assert dets[s] >= dets.max() * (1 - 1e-4), (dim, i, t)
                sel.append(s)
                checked += 1
    assert checked > 150


def test_logdet_invariant():
    """sum of log gain over a row's DPP steps = slogdet(L[sel, sel]) in float64,
    within 8 x the worst deviation measured over these cases (absolute, in
    log units; measured worst 1.14e-5, WORST_LOGDET_DEV)."""
    worst = 0.0
    for c in F64_CASES:
        T, ids, scores = _f64_case(c)
        k, theta, raw = c[3], c[4], c[5]
        items, _, gain = fh.dpp_select(T, ids, scores, k, theta, 1e-3, raw_scores=raw,
                                       return_gain=True)
        for i in range(F64_ROWS):
            filled, L = R.kernel64(T, ids[i], scores[i], theta, raw)
            steps = int((gain[i] > 0).sum())
            assert (gain[i, :steps] > 0).all() and steps >= 1
            sel = [int(np.flatnonzero(ids[i] == it)[0]) for it in items[i, :steps]]
            sign, ld = np.linalg.slogdet(L[np.ix_(sel, sel)])
            assert sign > 0
            worst = max(worst, abs(float(np.log(gain[i, :steps].astype(np.float64)).sum()) - ld))
    print(f"worst log-det deviation {worst:.2e}")
    assert worst <= 8 * WORST_LOGDET_DEV


def test_exact_identities():
    rng = np.random.default_rng(7600)
    # scaled unit vectors, d >= pool: exactly orthogonal, r stays exactly 1
    pool, k, dim = 12, 7, 16
    T = np.zeros((pool, dim), np.float32)
    T[np.arange(pool), rng.permutation(dim)[:pool]] = 2.0 ** rng.integers(-3, 4, pool)
    ids = np.stack([rng.permutation(pool) for _ in range(5)]).astype(np.int32)
    scores = rng.standard_normal((5, pool)).astype(np.float32)
    for theta, raw in ((3.0, True), (3.0, False), (0.5, True)):
        items, sc, gain = fh.dpp_select(T, ids, scores, k, theta, 1e-3, raw_scores=raw,
                                        return_gain=True)
        order = np.argsort(-scores.astype(np.float64), 1, kind="stable")[:, :k]
        assert np.array_equal(items, np.take_along_axis(ids, order, 1))
        assert np.array_equal(bits(sc), bits(np.take_along_axis(scores, order, 1)))
        # gain = w_b to the bit: the same w as a pool of that one slot gives
        if raw:
            one = fh.dpp_select(T, items.reshape(-1, 1), sc.reshape(-1, 1), 1, theta, 1e-3,
                                raw_scores=True, return_gain=True)[2]
            assert np.array_equal(bits(gain.reshape(-1)), bits(one[:, 0]))
    items, sc, gain = fh.dpp_select(T, ids, scores, k, 0.0, 1e-3, return_gain=True)
    assert np.array_equal(items, ids[:, :k]) and (gain == 1.0).all()  # all tie: slot order
    # a duplicated id, and a zero item row: only in the fallback
    G = R.gauss_table(50, 6, 7601)
    G[9] = 0.0
    tw = np.array([[4, 5, 4, 9, 6, 7]], np.int32)
    ts = np.array([[3.0, 2.5, 2.75, 5.0, 1.0, 0.5]], np.float32)
    items, sc, gain = fh.dpp_select(G, tw, ts, 6, 1.0, 1e-3, raw_scores=True, return_gain=True)
    at = {(int(it), float(s)): t for t, (it, s) in enumerate(zip(items[0], sc[0]))}
    first4, second4, zero = at[(4, 3.0)], at[(4, 2.75)], at[(9, 5.0)]
    assert gain[0, first4] > 0 and gain[0, second4] == 0 and gain[0, zero] == 0
    n_dpp = int((gain[0] > 0).sum())
    assert n_dpp == 4 and (gain[0, :4] > 0).all()
    assert items[0, 4:].tolist() == [4, 9]  # the fallback: ascending slots 2, 3
    # d = 5, pool 33, k 33: at most 5 DPP steps, then ascending slots at gain 0.0
    T5 = R.gauss_table(80, 5, 7602)
    X = rng.standard_normal((6, 5)).astype(np.float32)
    ids5, sc5 = R.top_pools(X, T5, 33)
    items, sc, gain = fh.dpp_select(T5, ids5, sc5, 33, 4.0, 1e-3, return_gain=True)
    for i in range(6):
        nd = int((gain[i] > 0).sum())
        assert 1 <= nd <= 5 and (gain[i, :nd] > 0).all()
        assert (bits(gain[i, nd:]) == 0).all()  # exactly +0.0
        rest = [int(np.flatnonzero(ids5[i] == it)[0]) for it in items[i, nd:]]
        assert rest == sorted(rest) and len(set(items[i].tolist())) == 33
    # fill beyond p, and gain = None changes no other byte
    holes = ids5.copy()
    holes[:, 4:9] = -1
    holes[:, 20:] = -1
    p = 15
    a = fh.dpp_select(T5, holes, sc5, 20, 4.0, 1e-3, return_gain=True)
    assert (a[0][:, :p] >= 0).all() and (a[0][:, p:] == -1).all()
    assert (a[1][:, p:] == -FLT_MAX).all() and (a[2][:, p:] == -FLT_MAX).all()
    b = fh.dpp_select(T5, holes, sc5, 20, 4.0, 1e-3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    none = np.full((2, 5), -1, np.int32)
    items, sc, gain = fh.dpp_select(T5, none, np.zeros((2, 5), np.float32), 3, return_gain=True)
    assert (items == -1).all() and (sc == -FLT_MAX).all() and (gain == -FLT_MAX).all()


def test_names_exported():
    def decls(path):
        txt = open(os.path.join(ROOT, "include", path)).read()
        return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    core, model = decls("frecsys_hip.h"), decls("frecsys_model.h")
    assert re.search(r"int frecsys_recommend_dpp\(frecsys_ctx\* ctx, int32_t side,[^;]*"
                     r"int32_t k, int32_t pool, float theta, float eps, int32_t flags,[^;]*"
                     r"float\* gain\);", core)
    assert re.search(r"int frecsys_diversify_dpp\(frecsys_ctx\* ctx, const int32_t\* lists,[^;]*"
                     r"int32_t pool, int32_t k, float theta, float eps,\s*int32_t flags,[^;]*"
                     r"float\* gain\);", core)
    assert re.search(r"int frecsys_dpp_select\(const float\* item_table, int64_t n_items, "
                     r"int32_t dim, int64_t ld,[^;]*float theta, float eps, int32_t flags,[^;]*"
                     r"float\*\s*gain\);", core)
    core_names = {"frecsys_recommend_dpp", "frecsys_diversify_dpp", "frecsys_dpp_select"}
    model_names = {"frecsys_model_recommend_dpp", "frecsys_model_recommend_dpp_fold_in",
                   "frecsys_model_diversify_dpp"}
    for name in model_names:
        assert re.search(r"int %s\(frecsys_model\* m,[^;]*float theta, float eps,[^;]*"
                         r"float\* gain\);" % name, model), name
    assert core_names <= set(fh.EXPORTS) and model_names <= set(fh.MODEL_EXPORTS)
    lib, ml = fh.load_library(), fh.load_model_library()
    for name in core_names:
        assert getattr(lib, name) is not None
    for name in model_names:
        assert getattr(ml, name) is not None
    assert callable(fh.dpp_select)
    assert callable(fh.Context.recommend_dpp) and callable(fh.Context.diversify_dpp)
    for name in ("recommend_dpp", "recommend_dpp_fold_in", "diversify_dpp"):
        assert callable(getattr(fh.Model, name))


def test_rejections():
    lib = fh.load_library()
    T = np.ones((10, 4), np.float32)
    ids = np.zeros((2, 8), np.int32)
    sc = np.zeros((2, 8), np.float32)
    items = np.zeros((2, 8), np.int32)
    out = np.zeros((2, 8), np.float32)
    P = fh._ptr

    def select(k=3, pool=8, theta=4.0, eps=1e-3, flags=0, n=2, tab=T, n_items=10, dim=4, ld=4,
               lists=ids, scores=sc, o_items=items, o_scores=out):
        return lib.frecsys_dpp_select(P(tab), n_items, dim, ld, P(lists), P(scores), n, pool, k,
                                      theta, eps, flags, P(o_items), P(o_scores), None)

    assert select() == fh.OK
    assert select(theta=0.0, eps=1.0) == fh.OK
    bad = [dict(k=0), dict(k=9), dict(pool=0), dict(pool=1025, k=1), dict(theta=-0.01),
           dict(theta=float("inf")), dict(theta=float("nan")), dict(eps=0.0), dict(eps=-1e-3),
           dict(eps=1.0001), dict(eps=float("nan")), dict(flags=1), dict(flags=4), dict(n=-1),
           dict(o_items=None), dict(o_scores=None), dict(tab=None), dict(lists=None),
           dict(scores=None), dict(n_items=0), dict(dim=0), dict(ld=3)]
    for kw in bad:
        assert select(**kw) == fh.ERR_INVALID, kw
    for kw in bad:  # zero rows are fine only with sound arguments
        if "n" not in kw and not ({"o_items", "o_scores", "tab", "lists", "scores", "n_items",
                                   "dim", "ld"} & set(kw)):
            assert select(n=0, **kw) == fh.ERR_INVALID, kw
    canary = items.copy()
    assert select(n=0, o_items=None, o_scores=None, lists=None, scores=None) == fh.OK
    assert np.array_equal(items, canary)
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
    assert lib.frecsys_diversify_dpp(None, P(ids), P(sc), 2, 8, 3, 4.0, 1e-3, 0, P(items), P(out),
                                     None) == fh.ERR_INVALID
    assert lib.frecsys_recommend_dpp(None, 0, None, 2, 3, 8, 4.0, 1e-3, 0, None, P(items), P(out),
                                     None) == fh.ERR_INVALID
    ml = fh.load_model_library()
    assert ml.frecsys_model_recommend_dpp(None, None, 0, 3, 8, 4.0, 1e-3, 0, 0, None, None, None,
                                          None) == fh.ERR_INVALID
    assert ml.frecsys_model_diversify_dpp(None, None, None, 0, 8, 3, 4.0, 1e-3, 0, None, None,
                                          None) == fh.ERR_INVALID
    with pytest.raises(fh.FrecsysError):
        fh.dpp_select(T, ids, sc, 9)
    with pytest.raises(fh.FrecsysError):
        fh.dpp_select(T, ids, sc, 3, eps=0.0)
