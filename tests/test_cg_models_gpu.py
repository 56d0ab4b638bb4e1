"""--use_cg through the C++ host layer: run_model on the ML-1M fixture with
the reference tests' settings (d = 8, 10 epochs) passes the reference's own
gates -- NDCG@20 >= 0.2 (ials_test.cc:45, safer2_test.cc:99), SAFER2's mean
dual weight within alpha +- 0.02 after every epoch (safer2_test.cc:135) --
and the model C-ABI trains and recommends with a 3-iteration cap."""
import os
import re
import subprocess

import numpy as np
import pytest

import frecsys_hip as fh
from conftest import ML1M, PKG

pytestmark = pytest.mark.gpu

BIN = os.path.join(PKG, "bin")
TRAIN = os.path.join(ML1M, "train.csv")
VTR = os.path.join(ML1M, "validation_tr.csv")
VTE = os.path.join(ML1M, "validation_te.csv")


def _run_model(args, timeout=600):
    cmd = [os.path.join(BIN, "run_model"), "--train_data", TRAIN, "--test_train_data", VTR,
           "--test_test_data", VTE, "--seed", "1", "--print_train_stats", "0",
           "--use_cg", "1"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _ndcg20(log):
    tail = log[log.rindex("Validation Results"):]
    m = re.search(r"Mean NDCG@20=([0-9.]+)", tail)
    assert m, tail[-2000:]
    return float(m.group(1))


def test_gate_ials_use_cg():  # ials_test.cc:17-45 with use_cg
    log = _run_model(["--model_name", "ials", "--dim", "8", "--uobs_weight", "0.1",
                      "--l2_reg", "0.003", "--epoch", "10"])
    nd = _ndcg20(log)
    print(f"iALS --use_cg NDCG@20 = {nd}")
    assert nd >= 0.2
    assert len(re.findall(r"Epoch: \d+, Timer: Train=\d+", log)) == 10


def test_gate_safer2_use_cg():  # safer2_test.cc:17-32, 66-99, 135 with use_cg
    log = _run_model(["--model_name", "safer2", "--dim", "8", "--uobs_weight", "0.004",
                      "--l2_reg", "0.004", "--bandwidth", "0.15", "--use_epanechnikov", "0",
                      "--xi_iterations", "5", "--pd_iterations", "1", "--epoch", "10",
                      "--print_var_stats", "1", "--cg_error_tolerance", "1e-10",
                      "--cg_max_iterations", "100"])
    nd = _ndcg20(log)
    means = [float(x) for x in re.findall(r"Min: [0-9.]+, Mean: ([0-9.]+), Max", log)]
    print(f"SAFER2 --use_cg NDCG@20 = {nd}, mean omega per epoch {means}")
    assert nd >= 0.2
    assert len(means) == 10
    assert all(abs(m - 0.3) <= 0.02 for m in means), means


def test_model_trains_and_recommends_with_iteration_cap(ml1m):
    tr, _, _ = ml1m
    m = fh.Model("ials", tr.users, tr.items, dim=32, stdev=0.1, seed=1, l2_reg=0.003,
                 uobs_weight=0.1, print_train_stats=False, use_cg=True, cg_max_iterations=3)
    ctx = m.context()
    m.train(2)
    # every solved row ran to the cap of 3 (tolerance 1e-10 is not reached in 3)
    it = ctx.cg_iterations(fh.SIDE_ITEM)
    up, uc = tr.by_user()
    ip, ic = tr.by_item()
    assert (it[np.diff(ip) > 0] == 3).all() and (it[np.diff(ip) == 0] == -1).all()
    n_solved = int((np.diff(up) > 0).sum() + (np.diff(ip) > 0).sum())
    assert ctx.counter("cg_iterations") == 2 * 3 * n_solved
    assert ctx.counter("cg_unconverged") == 2 * n_solved
    assert ctx.timing("solve_user.cg")[1] == 2 and ctx.timing("solve_user.dspace")[1] == 0
    U = ctx.get_embeddings(fh.SIDE_USER)
    V = ctx.get_embeddings(fh.SIDE_ITEM)
    assert np.isfinite(U).all() and np.isfinite(V).all()
    users = np.arange(0, m.n_users, 97)
    users = users[np.diff(up)[users] > 0]
    items, scores = m.recommend(users, 10)
    assert items.shape == (len(users), 10) and (items >= 0).all()
    S = U[users].astype(np.float64) @ V.astype(np.float64).T
    for i, u in enumerate(users):
        assert not set(items[i].tolist()) & set(uc[up[u]:up[u + 1]].tolist())
        np.testing.assert_allclose(scores[i], S[i, items[i]], rtol=0, atol=2e-6 * np.abs(S).max())
        assert np.all(np.diff(scores[i]) <= 0)
    # an inexact ALS epoch still fits: the truncated model ranks a user's
    # training items far above chance (mean score of seen vs all items)
    seen = np.mean([S[i, uc[up[u]:up[u + 1]]].mean() for i, u in enumerate(users)])
    assert seen > S.mean() + 0.1
    m.close()
