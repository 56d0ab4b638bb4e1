#!/usr/bin/env python3
"""Cost of an evaluation through frecsys_rank_metrics against what the library
offered before it: frecsys_recommend's lists copied to the host and the
metrics computed there (frecsys_list_metrics).  Rows loaded as the EVAL side,
fold-in history excluded, k_list (5, 10, 20, 50, 100), 1..40 random
ground-truth items per row; random N(0, d^-1/2) tables.  One warm-up, then the
median / min / max of 5 repetitions of
  rank_metrics   host clock around Context.rank_metrics, and the library's
                 timers "recommend" (the scan) and "rank_metrics" (the metric
                 kernel) inside it;
  recommend      host clock around Context.recommend(k = 100) on the same
                 rows, and its "recommend" timer;
  list_metrics   host clock around fh.list_metrics on those lists.

  a  all 116,677 rows x 20,108 items, d = 256 (the synthetic ML-20M CSR
     bench.py builds)
  b  its first 10,000 rows (a validation fold's size)

Usage: evaluate_bench.py [a|b ...] [--out FILE]
Prints one JSON line per case, times in ms.  The yardstick is recommend in the
same run: rank_metrics launches the same scan plus one small kernel and copies
less back, so its wall time is expected within recommend's own spread
(max - min), or below it.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402
from frecsys_hip.data import SHAPES, synthetic  # noqa: E402

K_LIST, REPS = (5, 10, 20, 50, 100), 5


def _tables(rows, items, dim, seed):
    rng = np.random.default_rng(seed)
    s = dim ** -0.25
    X = rng.standard_normal((rows, dim), dtype=np.float32) * np.float32(s)
    V = rng.standard_normal((items, dim), dtype=np.float32) * np.float32(s)
    return X, V


def _ground_truth(rows, items, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 41, rows)
    gp = np.concatenate([[0], np.cumsum(g)]).astype(np.int64)
    return gp, rng.integers(0, items, int(gp[-1])).astype(np.int32)


def _stat(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def _timed(ctx, keys, call):
    call()  # warm-up: allocations, code load
    wall, lib = [], {k: [] for k in keys}
    for _ in range(REPS):
        ctx.timing_reset()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for k in keys:
            lib[k].append(ctx.timing(k)[0])
    return wall, lib


def run_case(name, X, V, ep, ec):
    rows, dim = X.shape
    items = V.shape[0]
    gp, gi = _ground_truth(rows, items, 11)
    ctx = fh.Context(dim, 1, items)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, ep, ec)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    out = {}
    rm_wall, rm_lib = _timed(ctx, ("recommend", "rank_metrics"), lambda: out.update(
        m=ctx.rank_metrics(fh.SIDE_EVAL, K_LIST, gp, gi)))
    batches = ctx.timing("rank_metrics")[1]
    rc_wall, rc_lib = _timed(ctx, ("recommend",), lambda: out.update(
        r=ctx.recommend(fh.SIDE_EVAL, max(K_LIST))))
    ctx.close()
    lm_wall = []
    for i in range(REPS + 1):
        t0 = time.perf_counter()
        host = fh.list_metrics(out["r"][0], gp, gi, K_LIST)
        if i:
            lm_wall.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(out["m"][0].view(np.uint32), host[0].view(np.uint32)) and
                np.array_equal(out["m"][1].view(np.uint32), host[1].view(np.uint32)))
    res = {
        "case": name, "rows": rows, "items": items, "dim": dim, "k_list": list(K_LIST),
        "ground_truth_ids": int(gp[-1]), "row_batches": batches,
        "rank_metrics_wall_ms": _stat(rm_wall),
        "rank_metrics_scan_ms": _stat(rm_lib["recommend"]),
        "rank_metrics_kernel_ms": _stat(rm_lib["rank_metrics"]),
        "recommend_wall_ms": _stat(rc_wall),
        "recommend_scan_ms": _stat(rc_lib["recommend"]),
        "list_metrics_host_ms": _stat(lm_wall),
        "bitwise_equal_to_host": same,
        "mean_ndcg": [float(x) for x in out["m"][1].astype(np.float64).mean(axis=0)],
    }
    res["slower_than_recommend_by_ms"] = (res["rank_metrics_wall_ms"]["median"] -
                                          res["recommend_wall_ms"]["median"])
    res["recommend_spread_ms"] = res["recommend_wall_ms"]["max"] - res["recommend_wall_ms"]["min"]
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    cases = args or ["a", "b"]
    up, uc, ip, _ = synthetic(SHAPES["ml20m"])
    nu, ni = len(up) - 1, len(ip) - 1
    X, V = _tables(nu, ni, 256, 1)
    results = []
    if "a" in cases:
        results.append(run_case("a", X, V, up, uc))
        print(json.dumps(results[-1]), flush=True)
    if "b" in cases:
        n = 10_000
        results.append(run_case("b", X[:n], V, up[:n + 1], uc[:up[n]]))
        print(json.dumps(results[-1]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
