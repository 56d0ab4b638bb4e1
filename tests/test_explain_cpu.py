"""The float64 reference of frecsys_explain (tests/explain_ref.py) checked
against itself, the float32 rounding of the kernel's steps bounded on every
fixture the GPU tests use, and the names the feature adds.

test_reference_is_consistent       column sums = scores = v_t . x, x from
                                   numpy_ref's float64 direct solve.
test_top_of_tie_rule               a constructed tie, a short history, -0.0.
test_float32_steps_within_quarter  assemble / Cholesky / substitute / second
                                   pass in float32: per pair < TOL_ROW / 4.
test_names_exported                headers, EXPORTS / MODEL_EXPORTS, methods.
"""
import os
import re

import numpy as np
import pytest

import cg_ref as C
import explain_ref as X
import frecsys_hip as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, d) for d in X.DIMS for k in X.KINDS]
IDS = [f"{'ials' if k == C.KIND_IALS else 'u'}-d{d}" for k, d in CASES]


def test_fixture_covers_the_seams():
    hs = {h for h, _ in X.ROWS}
    ms = {m for _, m in X.ROWS}
    assert {0, 1, 31, 32, 33, X.CHUNK - 1, X.CHUNK, X.CHUNK + 1, 300, 2 * X.CHUNK + 5} <= hs
    assert {0, 1, 31, 32, 33, 70} <= ms
    assert min(h for h in hs if h) < 5 <= max(X.TOPS)  # a row shorter than a `top`
    case = X.get_case(C.KIND_IALS, 20)
    inside = repeated = 0
    for e in range(case.n_rows):
        t = case.targets(e)
        inside += len(set(t.tolist()) & set(case.hist(e).tolist()))
        repeated += len(t) - len(set(t.tolist()))
    assert inside > 0 and repeated > 0
    assert X.DIMS == (8, 20, 64, 100, 200, 256)
    assert [C.padded_dim(d) for d in X.DIMS] == [8, 32, 64, 128, 224, 256]


@pytest.mark.parametrize("kind,dim", CASES, ids=IDS)
def test_reference_is_consistent(kind, dim):
    case = X.get_case(kind, dim)
    direct = C.direct_side(case)  # numpy_ref's float64 solve of the same entities
    for e, (contrib, score, x) in enumerate(case.ref):
        h, m = X.ROWS[e]
        assert contrib.shape == (h, m) and score.shape == (m,)
        if h == 0:
            assert not score.any()
            continue
        V = case.X[case.targets(e)].astype(np.float64)
        np.testing.assert_allclose(contrib.sum(0), score, rtol=0, atol=1e-13)
        scale = np.linalg.norm(V, axis=1) * np.linalg.norm(direct[e])
        assert (np.abs(score - V @ direct[e]) <= 1e-10 * scale + 1e-300).all()
        assert np.linalg.norm(x - direct[e]) <= 1e-10 * np.linalg.norm(direct[e])


def test_top_of_tie_rule():
    full = np.array([0.5, 2.0, -1.0, 2.0, 0.5, 3.0], np.float32)
    pos, val = X.top_of(full, 4)
    assert pos.tolist() == [5, 1, 3, 0]  # 2.0 twice: the earlier position first
    assert val.tolist() == [3.0, 2.0, 2.0, 0.5]
    pos, val = X.top_of(full, 8)  # fill behind the history length
    assert pos.tolist() == [5, 1, 3, 0, 4, 2, -1, -1] and val[6:].tolist() == [0.0, 0.0]
    pos, _ = X.top_of(np.array([-0.0, 0.0, -0.0], np.float32), 3)
    assert pos.tolist() == [0, 1, 2]  # -0.0 ties with +0.0
    pos, val = X.top_of(np.zeros(0, np.float32), 2)
    assert pos.tolist() == [-1, -1] and val.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("kind,dim", CASES, ids=IDS)
def test_float32_steps_within_quarter(kind, dim):
    """Measured on these fixtures: worst 2e-5 (dim 200), <= 1e-5 elsewhere."""
    case = X.get_case(kind, dim)
    f32 = X.explain_case(case, np.float32)
    worst = 0.0
    for e, (contrib, score, x) in enumerate(case.ref):
        if contrib.size == 0:
            continue
        assert f32[e][0].dtype == np.float32
        worst = max(worst, float(X.pair_rel_err(f32[e][0], contrib).max()))
    print(f"float32 steps, worst pair rel err {worst:.2e}")
    assert worst < X.TOL_ROW / 4


def test_names_exported():
    def decls(path):
        txt = open(os.path.join(ROOT, "include", path)).read()
        return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    core, model = decls("frecsys_hip.h"), decls("frecsys_model.h")
    assert re.search(r"int frecsys_explain\(frecsys_ctx\* ctx, int32_t side,\s*"
                     r"const frecsys_solve_params\* params,[^;]*int32_t top,[^;]*float\* full\);",
                     core)
    assert re.search(r"int frecsys_model_explain\(frecsys_model\* m, const int64_t\* users,"
                     r"[^;]*float\* full\);", model)
    assert re.search(r"int frecsys_model_explain_fold_in\(frecsys_model\* m, "
                     r"const int64_t\* hist_ptr,[^;]*float\* full\);", model)
    assert "frecsys_explain" in fh.EXPORTS
    assert {"frecsys_model_explain", "frecsys_model_explain_fold_in"} <= set(fh.MODEL_EXPORTS)
    assert fh.load_library().frecsys_explain is not None
    ml = fh.load_model_library()
    assert ml.frecsys_model_explain is not None and ml.frecsys_model_explain_fold_in is not None
    assert callable(fh.Context.explain)
    assert callable(fh.Model.explain) and callable(fh.Model.explain_fold_in)
    raw = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "frecsys_model.h")).read())
    assert "not frecsys_model_score's U[user] . V[item]" in raw
