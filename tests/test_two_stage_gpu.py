"""frecsys_recommend_two_stage on the GPU (csrc/twostage.hip behind
csrc/serve.hip) against frecsys_recommend, bit for bit, and against the
float64 model of tests/two_stage_ref.py.

test_exact_tables (G1)       integer tables (bf16-exact, every sum exact in
                             fp32): the pools are recommend(k = pool) and the
                             lists recommend(k), bit for bit on every row --
                             with and without a mask and the history, repeated
                             rows, k and pool above the eligible count.  Pins
                             the scan's eligibility, threshold, tie and merge
                             logic with no tolerance.
test_gaussian_fixture (G2, G3, G7)  every row certified and recommend's bits;
                             the accumulator assumption |s^ - sum x^y^| <=
                             Dp 2^-23 sum |x^y^| in float64 on the pools; under
                             a random mask and the history every certified row
                             is recommend's.
test_cancellation (G3)       the same assumption where the products cancel.
test_near_tie (G4)           no row certifies; the lists are the pool's best by
                             score_pairs' bits; exact=True re-runs all 33 rows;
                             a mixed call falls back on a part of its rows.
test_knobs (G5)              item splits 1 / 3 / max and 1 MiB of workspace
                             change no output bit.
test_exclusions (G6)         a subnormal in the item table or a query row, a
                             NaN / inf in a query row: not certified, and
                             recommend's bits with exact=True.
test_eval_side_and_rejections (G8)
"""
import numpy as np
import pytest

import two_stage_ref as R

pytestmark = pytest.mark.gpu

import frecsys_hip as fh  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_lists(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))


def _same_all(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if g.dtype == np.float32:
            np.testing.assert_array_equal(_bits(g), _bits(w))
        else:
            np.testing.assert_array_equal(g, w)


def _ctx(U, V, hist=None, side=fh.SIDE_USER):
    ctx = fh.Context(U.shape[1], U.shape[0] if side == fh.SIDE_USER else 1, V.shape[0])
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    if hist is not None:
        ctx.load_csr(side, hist[0], hist[1])
    elif side == fh.SIDE_EVAL:
        ctx.load_csr(side, np.zeros(U.shape[0] + 1, np.int64), np.zeros(0, np.int32))
    ctx.set_embeddings(side, U)
    return ctx


def _accumulator_ratio(U, V, pool_items, pool_scores):
    """The worst |s^ - sum x^y^| / (Dp 2^-23 sum |x^y^|) over the filled pool
    slots, in float64."""
    Uh, Vh = R.bf16_round(U).astype(np.float64), R.bf16_round(V).astype(np.float64)
    dp = R.padded_dim(U.shape[1])
    worst = 0.0
    for r in range(U.shape[0]):
        ids = pool_items[r][pool_items[r] >= 0]
        prod = Vh[ids] * Uh[r][None, :]
        err = np.abs(pool_scores[r][:len(ids)].astype(np.float64) - prod.sum(1))
        worst = max(worst, float((err / (dp * 2.0 ** -23 * np.abs(prod).sum(1))).max()))
    return worst


@pytest.mark.parametrize("dim", (8, 96, 100, 150, 224, 256, 300))
def test_exact_tables(dim):
    rows, items = 70, 300
    U, V = R.integer_tables(dim, rows, items, 7400 + dim)
    hist = R.histories(rows, items, 7401)
    rng = np.random.default_rng(7402)
    half = (rng.random(items) < 0.5).astype(np.uint8)
    ten = np.zeros(items, np.uint8)
    ten[[3, 11, 57, 100, 127, 128, 200, 250, 298, 299]] = 1
    rep = np.array([5, 5, 69, 0, 5, 33, 69], np.int64)
    with _ctx(U, V, hist) as ctx:
        for k, pool, exclude, mask, rws in ((10, 64, True, None, None),
                                            (10, 64, False, None, None),
                                            (20, 128, True, half, None),
                                            (64, 64, False, half, None),
                                            (100, 400, True, None, None),  # pool > items
                                            (20, 64, True, ten, None),     # fill 10 < k
                                            (10, 33, True, None, rep)):
            kw = dict(rows=rws, exclude_history=exclude, item_mask=mask)
            items_, scores, cert, pi, ps = ctx.recommend_two_stage(
                fh.SIDE_USER, k, pool, exact=False, return_pool=True, **kw)
            _same_lists((pi, ps), ctx.recommend(fh.SIDE_USER, pool, **kw))
            want = ctx.recommend(fh.SIDE_USER, k, **kw)
            _same_lists((items_, scores), want)
            assert set(np.unique(cert)) <= {0, 1}
            if mask is ten:
                assert (cert == 1).all()  # a pool that is not full
                assert ((items_ >= 0).sum(1) <= 10).all() and (items_[:, 10:] == -1).all()
                assert (scores[:, 10:] == -R.FLT_MAX).all() and (ps[:, 10:] == -R.FLT_MAX).all()
            if pool > items:
                assert (cert == 1).all() and (pi[:, items:] == -1).all()


@pytest.mark.parametrize("i", range(len(R.FIXTURES)))
def test_gaussian_fixture(i):
    U, V, k, pool = R.fixture(i)
    rows, items = U.shape[0], V.shape[0]
    hist = R.histories(rows, items, 7500 + i)
    mask = (np.random.default_rng(7600 + i).random(items) < 0.7).astype(np.uint8)
    with _ctx(U, V, hist) as ctx:
        # G2: every item eligible, as in the model's claim
        got = ctx.recommend_two_stage(fh.SIDE_USER, k, pool, exclude_history=False, exact=False,
                                      return_pool=True)
        assert (got[2] == 1).all(), np.flatnonzero(got[2] != 1)
        _same_lists(got[:2], ctx.recommend(fh.SIDE_USER, k, exclude_history=False))
        # G3
        ratio = _accumulator_ratio(U, V, got[3], got[4])
        print(f"two-stage accumulator ratio, fixture {R.FIXTURES[i]}: {ratio:.4f}")
        assert ratio <= 1.0
        # G7: whatever is certified is recommend's list
        got = ctx.recommend_two_stage(fh.SIDE_USER, k, pool, item_mask=mask, exact=False)
        want = ctx.recommend(fh.SIDE_USER, k, item_mask=mask)
        c = got[2] == 1
        assert c.any()
        _same_lists((got[0][c], got[1][c]), (want[0][c], want[1][c]))
        # and with the fallback, every row
        got = ctx.recommend_two_stage(fh.SIDE_USER, k, pool, item_mask=mask)
        assert set(np.unique(got[2])) <= {1, 2}
        np.testing.assert_array_equal(got[2] == 1, c)
        _same_lists(got[:2], want)


@pytest.mark.parametrize("i", range(len(R.CANCEL)))
def test_cancellation(i):
    U, V, k, pool = R.cancellation(i)
    with _ctx(U, V) as ctx:
        got = ctx.recommend_two_stage(fh.SIDE_USER, k, pool, exclude_history=False,
                                      return_pool=True)
        _same_lists(got[:2], ctx.recommend(fh.SIDE_USER, k, exclude_history=False))
        ratio = _accumulator_ratio(U, V, got[3], got[4])
        print(f"two-stage accumulator ratio, cancellation {R.CANCEL[i]}: {ratio:.4f}")
        assert ratio <= 1.0


def test_near_tie():
    U, V, k, pool = R.near_tie()
    rows = U.shape[0]
    with _ctx(U, V) as ctx:
        want = ctx.recommend(fh.SIDE_USER, k, exclude_history=False)
        items, scores, cert = ctx.recommend_two_stage(fh.SIDE_USER, k, pool,
                                                      exclude_history=False, exact=False)
        assert (cert == 0).all()
        assert (items >= 0).all()
        pairs = ctx.score_pairs(fh.SIDE_USER, np.repeat(np.arange(rows), k), items.reshape(-1))
        np.testing.assert_array_equal(_bits(scores).reshape(-1), _bits(pairs))
        assert (items != want[0]).any()  # the true top-k did leave the pools
        before = ctx.counter("two_stage_fallback_rows")
        got = ctx.recommend_two_stage(fh.SIDE_USER, k, pool, exclude_history=False)
        _same_lists(got[:2], want)
        assert (got[2] == 2).all()
        assert ctx.counter("two_stage_fallback_rows") == before + rows
        assert ctx.timing("two_stage.fallback")[1] >= 1
    # a call whose rows fall back in part
    U, V, k, pool, certifying = R.mixed()
    with _ctx(U, V) as ctx:
        want = ctx.recommend(fh.SIDE_USER, k, exclude_history=False)
        c0, f0 = ctx.counter("two_stage_certified"), ctx.counter("two_stage_fallback_rows")
        got = ctx.recommend_two_stage(fh.SIDE_USER, k, pool, exclude_history=False)
        np.testing.assert_array_equal(got[2], np.where(certifying, 1, 2))
        _same_lists(got[:2], want)
        assert ctx.counter("two_stage_certified") == c0 + int(certifying.sum())
        assert ctx.counter("two_stage_fallback_rows") == f0 + int((~certifying).sum())
        # scores not asked for, rows given
        rws = np.arange(rows - 1, -1, -1)
        r = None
        items = np.zeros((rows, k), np.int32)
        rr = np.ascontiguousarray(rws, np.int64)
        assert ctx.lib.frecsys_recommend_two_stage(
            ctx.h, fh.SIDE_USER, fh._ptr(rr), rows, k, pool, fh.TS_EXACT, r, fh._ptr(items), None,
            None, None, None) == fh.OK
        np.testing.assert_array_equal(items, want[0][::-1])


def test_knobs(monkeypatch):
    U, V, k, pool = R.fixture(3)
    Un, Vn, _, _, _ = R.mixed()
    hist = R.histories(U.shape[0], V.shape[0], 7700)
    with _ctx(U, V, hist) as ctx, _ctx(Un, Vn) as mixed:
        def run():
            return (ctx.recommend_two_stage(fh.SIDE_USER, k, pool, exact=False, return_pool=True) +
                    mixed.recommend_two_stage(fh.SIDE_USER, 10, 64, exclude_history=False,
                                              return_pool=True))
        want = run()
        for splits, ws in (("1", None), ("3", None), ("64", None), (None, "1"), ("3", "1")):
            for name, v in (("FRECSYS_RECOMMEND_SPLITS", splits), ("FRECSYS_RECOMMEND_WS_MB", ws)):
                if v is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, v)
            _same_all(run(), want)
            if splits == "1":
                assert ctx.counter("recommend_splits") == 1


def test_exclusions():
    U, V, k, pool = R.fixture(2)
    tiny = np.float32(1e-39)  # an fp32 subnormal whose bf16 is subnormal too
    assert 0 < float(fh.bf16_round(np.array([tiny]))[0]) < 2.0 ** -126

    def run(Uq, Vq):
        with _ctx(Uq, Vq) as ctx:
            want = ctx.recommend(fh.SIDE_USER, k, exclude_history=False)
            cert = ctx.recommend_two_stage(fh.SIDE_USER, k, pool, exclude_history=False,
                                           exact=False)[2]
            got = ctx.recommend_two_stage(fh.SIDE_USER, k, pool, exclude_history=False)
            _same_lists(got[:2], want)
            np.testing.assert_array_equal(got[2], np.where(cert == 1, 1, 2))
            return cert
    assert (run(U, V) == 1).all()
    V2 = V.copy()
    V2[5, 3] = tiny
    assert (run(U, V2) == 0).all()  # the item table: no row
    U2 = U.copy()
    U2[4, 2] = -tiny
    U2[7, 0] = np.nan
    U2[9, 1] = np.inf
    U2[11, 5] = -np.inf
    cert = run(U2, V)
    bad = np.zeros(len(U), bool)
    bad[[4, 7, 9, 11]] = True
    np.testing.assert_array_equal(cert == 1, ~bad)
    # a value that rounds to zero is none: 1e-45 -> 0
    U3 = U.copy()
    U3[4, 2] = np.float32(1e-45)
    assert (run(U3, V) == 1).all()


def test_eval_side_and_rejections():
    U, V, k, pool = R.fixture(1)
    rows, items = U.shape[0], V.shape[0]
    hist = R.histories(rows, items, 7800)
    with _ctx(U, V, hist) as a, _ctx(U, V, hist, side=fh.SIDE_EVAL) as b:
        for exact in (False, True):
            _same_all(b.recommend_two_stage(fh.SIDE_EVAL, k, pool, exact=exact, return_pool=True),
                      a.recommend_two_stage(fh.SIDE_USER, k, pool, exact=exact, return_pool=True))
        _same_lists(b.recommend_two_stage(fh.SIDE_EVAL, k)[:2], b.recommend(fh.SIDE_EVAL, k))
        # pool = 0 is the default pool
        _same_all(a.recommend_two_stage(fh.SIDE_USER, k, 0, return_pool=False),
                  a.recommend_two_stage(fh.SIDE_USER, k, fh.default_two_stage_pool(k)))
    with _ctx(U, V) as ctx:  # no CSR loaded
        lib, P = ctx.lib, fh._ptr
        out_i = np.full((3, 4), 77, np.int32)
        out_s = np.full((3, 4), 7.0, np.float32)
        cert = np.full(3, 9, np.uint8)
        pi = np.full((3, 8), 77, np.int32)
        ps = np.full((3, 8), 7.0, np.float32)
        far = np.array([0, 1, rows], np.int64)
        neg = np.array([0, -1, 2], np.int64)

        def call(side=fh.SIDE_USER, r=None, n=3, k_=4, pool_=8, flags=0, o=out_i):
            return lib.frecsys_recommend_two_stage(
                ctx.h, side, None if r is None else P(r), n, k_, pool_, flags, None,
                None if o is None else P(o), P(out_s), P(cert), P(pi), P(ps))
        before = (ctx.counter("two_stage_certified"), ctx.counter("two_stage_fallback_rows"),
                  ctx.timing("two_stage.convert")[1], ctx.timing("two_stage.scan")[1])
        for kw in (dict(side=fh.SIDE_ITEM), dict(side=3), dict(k_=0), dict(k_=9), dict(k_=1025),
                   dict(pool_=1025), dict(pool_=-1), dict(k_=0, pool_=0), dict(flags=4),
                   dict(flags=8 | fh.TS_EXACT), dict(r=far), dict(r=neg), dict(n=-1),
                   dict(n=rows + 1), dict(o=None), dict(flags=fh.REC_EXCLUDE_HISTORY)):
            assert call(**kw) == fh.ERR_INVALID, kw
        assert call(n=0) == fh.OK and call(n=0, o=None) == fh.OK
        assert call(n=0, k_=0) == fh.ERR_INVALID
        assert (out_i == 77).all() and (out_s == 7.0).all() and (cert == 9).all()
        assert (pi == 77).all() and (ps == 7.0).all()
        assert before == (ctx.counter("two_stage_certified"),
                          ctx.counter("two_stage_fallback_rows"),
                          ctx.timing("two_stage.convert")[1], ctx.timing("two_stage.scan")[1])
        assert call() == fh.OK
        assert ctx.timing("two_stage.scan")[1] == before[3] + 1
        assert ctx.timing("two_stage.select")[1] >= 1
        flops, nbytes, ent, _ = ctx.work("two_stage.scan")
        dh = max(16, R.padded_dim(U.shape[1]))
        assert flops == 2.0 * 3 * items * U.shape[1]
        assert nbytes == (3 + items) * dh * 2 + 8 * 3 * 8 and ent == 3
        ctx.release_workspaces()
        assert call() == fh.OK  # the image is built again
