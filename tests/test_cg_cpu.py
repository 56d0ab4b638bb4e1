"""The conjugate-gradient path without a GPU: the numpy reference of
tests/cg_ref.py, the fixtures of tests/test_cg_gpu.py, and the new C-ABI /
model surface (declared, exported, defaults, rejections before any device
call)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cg_ref as C
import frecsys_hip as fh
from conftest import ROOT, rel_rows

CASES = C.gpu_cases()
IDS = [c[0] for c in CASES]
ARGS = [c[1] for c in CASES]


@pytest.mark.parametrize("args", ARGS, ids=IDS)
def test_cg_ref_converges_to_direct_solve(args):
    """cg_ref at 100 iterations (tolerance 1e-10, and 0) = the float64 direct
    solve: residual 1e-10 ||b|| times cond(A) <~ 100 is far below 1e-7."""
    case = C.get_case(args)
    assert rel_rows(case.conv, case.direct).max() < 1e-7
    assert case.conv_iters.max() < 100
    x0, it0, _ = C.cg_side(case, 100, 0.0)
    assert rel_rows(x0, case.direct).max() < 1e-9
    solved = np.diff(case.ptr) > 0
    assert (it0[~solved] == -1).all() and (it0[solved] >= case.conv_iters[solved]).all()
    for e in case.empty:
        np.testing.assert_array_equal(case.conv[e], case.E0[e].astype(np.float64))


@pytest.mark.parametrize("args", ARGS, ids=IDS)
def test_float32_recurrence_stays_within_a_quarter_of_the_bar(args):
    """A float32 numpy CG with the same recurrence differs from the float64
    one by < TOL_ROW / 4 on every fixture the GPU tests use: truncated
    iterates (1, 2, 5), the converged solve against the direct one, and the
    tolerance-1e-3 stop (true residual <= 2e-3 with float32 arithmetic)."""
    case = C.get_case(args)
    _, _, t32 = C.cg_side(case, max(C.CAPS), 0.0, np.float32, C.CAPS)
    for cap in C.CAPS:
        assert rel_rows(t32[cap], case.trunc[cap]).max() < C.TOL_ROW / 4
    x32, it32, _ = C.cg_side(case, 100, 1e-10, np.float32)
    assert rel_rows(x32, case.direct).max() < C.TOL_ROW / 4
    assert it32.max() < 100
    x3, it3, _ = C.cg_side(case, 100, 1e-3, np.float32)
    assert C.residual_side(case, x3).max() <= 2e-3
    if case.n_rows > 1:  # the stopping-rule test needs rows that stop at different counts
        assert len(set(it3[it3 >= 0].tolist())) > 1
    # the truncated iterates are far from the exact solve (5 - 80 %)
    solved = np.diff(case.ptr) > 0
    assert rel_rows(case.trunc[1], case.direct)[solved].max() > 0.05


def test_fixtures_cover_the_shapes():
    for d in C.DIMS:
        c = C.row_chunk(d)
        lens = set(np.diff(C.get_case((C.KIND_IALS, C.SIDE_USER, d, 70, False)).ptr).tolist())
        assert {0, 1, 3, 64, 129, 300, c - 1, c, c + 1, C.COOP_ROWS, C.COOP_ROWS + 1} <= lens
        assert len(C.get_case((C.KIND_IALS, C.SIDE_USER, d, 33, False)).empty) == 2
        assert C.padded_dim(d) == fh.padded_dim(d)
    assert [C.row_chunk(d) for d in C.DIMS] == [256, 64, 32, 16, 8, 8]
    v = C.get_case((C.KIND_V, C.SIDE_ITEM, 64, 70, True))
    assert np.diff(v.ptr)[0] == 300 and v.quirk  # the tail quirk's h


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return txt, set(re.findall(r"\b(frecsys_[a-z_0-9]+)\s*\(", txt))


def test_cg_symbols_declared_and_exported():
    txt, names = _declared("frecsys_hip.h")
    new = {"frecsys_solve_side_cg", "frecsys_cg_iterations"}
    assert new <= names and new <= set(fh.EXPORTS)
    assert re.search(r"int32_t\s+max_iterations;\s*float\s+tolerance;\s*}\s*frecsys_cg_params", txt)
    lib = fh.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", fh.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (frecsys_\w+)", out))
    for n in new:
        assert n in exported and getattr(lib, n) is not None
    assert ctypes.sizeof(fh._CgParams) == 8
    mtxt, _ = _declared("frecsys_model.h")
    # appended at the end of frecsys_model_config, in this order
    assert re.search(r"comm_id;\s*int32_t\s+use_cg;\s*float\s+cg_error_tolerance;\s*"
                     r"int32_t\s+cg_max_iterations;\s*}\s*frecsys_model_config", mtxt)
    assert [f[0] for f in fh._ModelConfig._fields_][-3:] == \
        ["use_cg", "cg_error_tolerance", "cg_max_iterations"]
    for name in ("solve_side_cg", "cg_iterations"):
        assert callable(getattr(fh.Context, name))


def test_model_config_cg_defaults():
    lib = fh.load_model_library()
    cfg = fh._ModelConfig()
    lib.frecsys_model_config_default(ctypes.byref(cfg))
    assert (cfg.use_cg, cfg.cg_max_iterations) == (0, 100)
    assert np.float32(cfg.cg_error_tolerance) == np.float32(1e-10)


def test_erm_mf_rejects_use_cg_before_any_device_call():
    u = np.array([0, 1, 1], np.int32)
    i = np.array([0, 0, 1], np.int32)
    with pytest.raises(fh.FrecsysError) as ei:
        fh.Model("erm_mf", u, i, dim=8, use_cg=True)
    assert ei.value.code == fh.ERR_UNSUPPORTED
    assert "BiCGSTAB" in str(ei.value)


def test_invalid_cg_parameters_rejected():
    u = np.array([0, 1, 1], np.int32)
    i = np.array([0, 0, 1], np.int32)
    for model in ("ials", "safer2"):
        for bad in (dict(cg_max_iterations=-1), dict(cg_error_tolerance=-1e-3),
                    dict(cg_error_tolerance=float("nan"))):
            with pytest.raises(fh.FrecsysError) as ei:
                fh.Model(model, u, i, dim=8, use_cg=True, **bad)
            assert ei.value.code == fh.ERR_INVALID, (model, bad)
        with pytest.raises(fh.FrecsysError) as ei:  # the CG kernel's limit, named
            fh.Model(model, u, i, dim=300, use_cg=True)
        assert ei.value.code == fh.ERR_UNSUPPORTED and "256" in str(ei.value)
    # the C entry points reject their arguments without a context
    lib = fh.load_library()
    cg = fh._CgParams(-1, 0.0)
    assert lib.frecsys_solve_side_cg(None, 0, None, ctypes.byref(cg)) == fh.ERR_INVALID
    assert lib.frecsys_cg_iterations(None, 0, None) == fh.ERR_INVALID
