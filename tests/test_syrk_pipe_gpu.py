"""The split-bf16 SYRK with its operand reads pipelined computes the same bits.

The pipelining (FRECSYS_SYRK_PIPE) moves LDS reads relative to
the MFMAs that consume them and changes no product, operand or order, so every
output table must hash to what the parent commit's library wrote on the same
hardware: tests/golden/syrk_pipe_parent_sha256.json, made by
scripts/syrk_pipe_hashes.py with that library (it records the commit; the
library was run twice there and every case was the same bytes both times).
test_seam_gpu.py bounds the same half-steps against float64; this file adds
that the bits did not move.

Cases (scripts/syrk_pipe_hashes.py): ials_user, ials_item, weighted_u and
weighted_v_quirk of tests/seam_data.py at dims 20, 64, 100, 200, 256 (T = 1,
2, 4, 7, 8) under test_seam_gpu's dspace, dspace_split and hspace_max
environments (hspace_max does not exist at Dp = 32, there as here), and the
two-epoch iALS trajectory of scripts/bitwise_epochs.py at d = 256 under the
default dispatch.  On a mismatch the worst row's relative error against the
float64 reference is printed, to tell "reordered" from "wrong".
"""
import json
import os
import sys

import numpy as np
import pytest

import seam_data as S
from conftest import ROOT, rel_rows

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import syrk_pipe_hashes as H  # noqa: E402

with open(H.GOLDEN) as _f:
    GOLD = json.load(_f)

_epochs = {}


def _clear_env(monkeypatch):
    # H._Env drops and restores FRECSYS_* itself; monkeypatch keeps pytest's
    # own view of the environment consistent with the other GPU tests
    for k in [k for k in os.environ if k.startswith("FRECSYS_")]:
        monkeypatch.delenv(k)


def test_golden_file_covers_the_cases():
    assert len(GOLD["commit"]) == 40
    assert sorted(GOLD["hashes"]) == sorted(H.case_ids())
    assert len(H.seam_cases()) == 4 * (5 + 5 + 4)


@pytest.mark.parametrize("key,dim,mode", H.seam_cases())
def test_seam_half_step_same_bits_as_parent(monkeypatch, key, dim, mode):
    _clear_env(monkeypatch)
    out = H.run_seam(key, dim, mode)
    got, want = H.digest(out), GOLD["hashes"][H.case_id(key, dim, mode)]
    if got != want:
        c = S.seam_case(key, dim)
        live = np.nonzero(c.h > 0)[0]
        err = rel_rows(out[live], S.reference(c)[live])
        w = live[int(np.argmax(err))]
        print(f"syrk_pipe {key} d={dim} {mode}: hash differs from {GOLD['commit'][:12]}; worst row "
              f"vs float64 {err.max():.3e} at h = {c.h[w]} ({c.labels[w]})")
    assert got == want


@pytest.mark.parametrize("table", ["U", "V"])
def test_two_epoch_trajectory_same_bits_as_parent(monkeypatch, table):
    _clear_env(monkeypatch)
    if not _epochs:
        U, V = H.run_epochs()
        _epochs.update(U=U, V=V)
    out = _epochs[table]
    got, want = H.digest(out), GOLD["hashes"][f"epochs/ials_d{H.EPOCH_DIM}/{table}"]
    if got != want:
        print(f"syrk_pipe epochs d={H.EPOCH_DIM} {table}: hash differs from {GOLD['commit'][:12]}; "
              f"finite {bool(np.isfinite(out).all())}, max |x| {np.abs(out).max():.3e}")
    assert got == want
