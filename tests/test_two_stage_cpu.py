"""Two-stage recommend without a GPU: the names, the host definitions
(frecsys_bf16_round, frecsys_two_stage_bound) against tests/two_stage_ref.py,
and the reference module's own claims about the fixtures the GPU tests use.

test_names_exported          the headers, fh.EXPORTS / MODEL_EXPORTS, the
                             Python names.
test_bf16_round_bits         fh.bf16_round against the numpy formula, bit for
                             bit: ties to even both ways, +-0, subnormals, the
                             largest finite value (-> inf), +-inf, NaN, 10^5
                             random bit patterns.
test_bound                   fh.two_stage_bound against the formula.
test_fixture_claims          for every Gaussian fixture the float64 model finds
                             the exact top-k inside the bf16 top-pool and the
                             row certified with a 1 % margin; for the near-tie
                             fixture no row can certify and the top-k leaves
                             the pool.  (A fixture change cannot make the GPU
                             tests vacuous.)
test_rejections              null context and bad host arguments.
"""
import os
import re

import numpy as np
import pytest

import two_stage_ref as R

import frecsys_hip as fh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_names_exported():
    def decls(path):
        txt = open(os.path.join(ROOT, "include", path)).read()
        return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    core, model = decls("frecsys_hip.h"), decls("frecsys_model.h")
    assert re.search(r"#define FRECSYS_TS_EXACT 2\b", core)
    assert re.search(r"int frecsys_recommend_two_stage\(frecsys_ctx\* ctx, int32_t side,[^;]*"
                     r"int32_t k, int32_t pool, int32_t flags,[^;]*uint8_t\* certified,[^;]*"
                     r"int32_t\* pool_items, float\* pool_scores\);", core)
    assert re.search(r"int frecsys_bf16_round\(const float\* in, int64_t n, float\* out\);", core)
    assert re.search(r"double frecsys_two_stage_bound\(int32_t dim, double query_norm, "
                     r"double item_norm_max\);", core)
    core_names = {"frecsys_recommend_two_stage", "frecsys_bf16_round", "frecsys_two_stage_bound"}
    model_names = {"frecsys_model_recommend_two_stage",
                   "frecsys_model_recommend_two_stage_fold_in"}
    for name in model_names:
        assert re.search(r"int %s\(frecsys_model\* m,[^;]*int32_t k,\s*int32_t pool, "
                         r"int32_t exact, int32_t exclude_seen,[^;]*uint8_t\* certified\);" % name,
                         model), name
    assert core_names <= set(fh.EXPORTS) and model_names <= set(fh.MODEL_EXPORTS)
    lib, ml = fh.load_library(), fh.load_model_library()
    for name in core_names:
        assert getattr(lib, name) is not None
    for name in model_names:
        assert getattr(ml, name) is not None
    assert fh.TS_EXACT == 2
    assert callable(fh.bf16_round) and callable(fh.two_stage_bound)
    assert callable(fh.Context.recommend_two_stage)
    for name in ("recommend_two_stage", "recommend_two_stage_fold_in"):
        assert callable(getattr(fh.Model, name))
    assert [fh.default_two_stage_pool(k) for k in (1, 16, 17, 100, 256, 1024)] == \
        [64, 64, 68, 400, 1024, 1024]


def test_bf16_round_bits():
    def f(*patterns):
        return np.array(patterns, np.uint32).view(np.float32)
    cases = f(
        0x3F808000, 0x3F818000,              # ties: down to even, up to even
        0xBF808000, 0xBF818000,
        0x3F808001, 0x3F807FFF,              # just above / below a tie
        0x00000000, 0x80000000,              # +-0
        0x00000001, 0x00008000, 0x00018000,  # subnormals: to 0, tie to 0, tie up
        0x007FFFFF, 0x807FFFFF,              # largest subnormal -> smallest normal
        0x7F7FFFFF, 0xFF7FFFFF,              # largest finite -> +-inf
        0x7F7F7FFF, 0x7F7F8000,              # below / at the tie under inf
        0x7F800000, 0xFF800000,              # +-inf
        0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF)  # NaNs
    got = fh.bf16_round(cases)
    np.testing.assert_array_equal(_bits(got), _bits(R.bf16_round(cases)))
    want = np.array([0x3F800000, 0x3F820000, 0xBF800000, 0xBF820000, 0x3F810000, 0x3F800000,
                     0x00000000, 0x80000000, 0x00000000, 0x00000000, 0x00020000,
                     0x00800000, 0x80800000, 0x7F800000, 0xFF800000, 0x7F7F0000, 0x7F800000,
                     0x7F800000, 0xFF800000], np.uint32)
    np.testing.assert_array_equal(_bits(got)[:len(want)], want)
    assert np.isnan(got[len(want):]).all()  # a NaN stays a NaN
    assert (_bits(got) & 0xFFFF == 0).all()
    rng = np.random.default_rng(7000)
    rnd = rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    np.testing.assert_array_equal(_bits(fh.bf16_round(rnd)), _bits(R.bf16_round(rnd)))
    mat = rnd[:600].reshape(20, 30)  # the shape is kept
    assert fh.bf16_round(mat).shape == (20, 30)
    # against the definition by value: the nearest bf16, never farther than half an ulp
    fin = rnd[np.isfinite(rnd) & (np.abs(rnd) < 1e38) & (np.abs(rnd) > 1e-37)].astype(np.float64)
    err = np.abs(fh.bf16_round(fin.astype(np.float32)).astype(np.float64) - fin)
    assert (err <= np.abs(fin) * 2.0 ** -8).all()
    assert fh.bf16_round(np.zeros(0, np.float32)).shape == (0,)


def test_bound():
    for dim in (1, 8, 9, 20, 100, 256, 257, 300, 1000, 1024):
        dp = R.padded_dim(dim)
        assert dp == fh.load_library().frecsys_padded_dim(dim)
        for xn, nm in ((1.0, 1.0), (0.98765, 1.2345), (0.0, 3.0), (1e-30, 1e30)):
            want = (2.0 ** -7 + 2.0 ** -16 + 3.0 * dp * 2.0 ** -23) * xn * nm
            assert fh.two_stage_bound(dim, xn, nm) == want == R.bound(dim, xn, nm)
    assert np.isnan(fh.two_stage_bound(0, 1.0, 1.0)) and np.isnan(fh.two_stage_bound(1025, 1.0, 1.0))
    assert np.isinf(fh.two_stage_bound(64, np.inf, 1.0))
    assert np.isnan(fh.two_stage_bound(64, np.nan, 1.0))


@pytest.mark.parametrize("i", range(len(R.FIXTURES)))
def test_fixture_claims(i):
    U, V, k, pool = R.fixture(i)
    dim, rows, items, k0, pool0 = R.FIXTURES[i]
    assert U.shape == (rows, dim) and V.shape == (items, dim) and (k, pool) == (k0, pool0)
    assert 1 <= k <= pool <= 1024 and pool < items
    m = R.model(U, V, k, pool)
    assert all(m["in_pool"]), np.flatnonzero(~np.array(m["in_pool"]))
    assert all(m["certifies"]), np.flatnonzero(~np.array(m["certifies"]))


def test_near_tie_claims():
    U, V, k, pool = R.near_tie()
    m = R.model(U, V, k, pool)
    assert all(m["cannot"]) and not any(m["certifies"])
    assert not any(m["in_pool"])


def test_mixed_claims():
    U, V, k, pool, certifying = R.mixed()
    m = R.model(U, V, k, pool)
    assert certifying.any() and (~certifying).any()
    np.testing.assert_array_equal(np.array(m["certifies"]), certifying)
    np.testing.assert_array_equal(np.array(m["cannot"]), ~certifying)


def test_cancellation_fixture():
    for i in range(len(R.CANCEL)):
        U, V, k, pool = R.cancellation(i)
        Uh, Vh = R.bf16_round(U).astype(np.float64), R.bf16_round(V).astype(np.float64)
        ratio = np.abs(Uh @ Vh.T) / (np.abs(Uh) @ np.abs(Vh).T)
        assert np.median(ratio) < 0.1  # the sums do cancel


def test_rejections():
    lib = fh.load_library()
    P = fh._ptr
    items = np.zeros((2, 3), np.int32)
    assert lib.frecsys_recommend_two_stage(None, 0, None, 2, 3, 8, 0, None, P(items), None, None,
                                           None, None) == fh.ERR_INVALID
    x = np.ones(4, np.float32)
    assert lib.frecsys_bf16_round(None, 4, P(x)) == fh.ERR_INVALID
    assert lib.frecsys_bf16_round(P(x), 4, None) == fh.ERR_INVALID
    assert lib.frecsys_bf16_round(P(x), -1, P(x)) == fh.ERR_INVALID
    assert lib.frecsys_bf16_round(None, 0, None) == fh.OK
    ml = fh.load_model_library()
    assert ml.frecsys_model_recommend_two_stage(None, None, 0, 3, 8, 1, 0, None, None, None,
                                                None) == fh.ERR_INVALID
    assert ml.frecsys_model_recommend_two_stage_fold_in(None, None, None, 0, 3, 8, 1, 0, None,
                                                        None, None, None) == fh.ERR_INVALID
