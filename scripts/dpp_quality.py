#!/usr/bin/env python3
"""What the DPP re-ranking buys on ML-1M (tests/golden/ml-1m): iALS at dim 64
after one epoch, the validation users folded in from validation_tr.csv, k = 20
from a pool of 200, history excluded.  ILD@20 (Model.list_quality) and
Recall@20 / NDCG@20 against validation_te.csv (fh.list_metrics) of
  recommend            the plain top 20
  mmr lam=0.7          recommend_diverse_fold_in
  dpp theta=0/2/4/8    recommend_dpp_fold_in, eps = 1e-3
and, for the DPP rows, the mean number of DPP steps before the fallback.

Usage: dpp_quality.py [--out FILE.jsonl]
Prints (and appends to FILE) one JSON line per configuration.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402
from frecsys_hip.data import Dataset  # noqa: E402

ML1M = os.path.join(ROOT, "tests", "golden", "ml-1m")
DIM, K, POOL = 64, 20, 200


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    tr = Dataset.from_csv(os.path.join(ML1M, "train.csv"))
    vt = Dataset.from_csv(os.path.join(ML1M, "validation_tr.csv"))
    ve = Dataset.from_csv(os.path.join(ML1M, "validation_te.csv"))
    ids, ep, ec = vt.compact_users()
    ids2, gp, gc = ve.compact_users()
    assert np.array_equal(ids, ids2)
    m = fh.Model("ials", tr.users, tr.items, dim=DIM, stdev=0.1, seed=1, l2_reg=0.003,
                 l2_reg_exp=1.0, uobs_weight=0.1, print_train_stats=False)
    m.initialize()
    m.train(1)
    runs = [("recommend", {}, lambda: m.recommend_fold_in(ep, ec, K)),
            ("mmr", {"lam": 0.7}, lambda: m.recommend_diverse_fold_in(ep, ec, K, POOL, 0.7))]
    for theta in (0.0, 2.0, 4.0, 8.0):
        runs.append(("dpp", {"theta": theta, "eps": 1e-3},
                     lambda theta=theta: m.recommend_dpp_fold_in(ep, ec, K, POOL, theta, 1e-3,
                                                                 return_gain=True)))
    for name, params, call in runs:
        got = call()
        q = m.list_quality(got[0], [K])
        recall, ndcg = fh.list_metrics(got[0], gp, gc, [K])
        res = {"bench": "dpp_quality", "data": "ml-1m", "model": "ials", "dim": DIM, "epochs": 1,
               "users": int(len(ids)), "k": K, "pool": POOL if name != "recommend" else K,
               "method": name, **params,
               "ild": float(np.asarray(q["ild"], np.float64).mean()),
               "recall": float(recall.mean(dtype=np.float64)),
               "ndcg": float(ndcg.mean(dtype=np.float64))}
        if name == "dpp":
            res["dpp_steps_mean"] = float((got[2] > 0).sum(1).mean())
        line = json.dumps(res)
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
