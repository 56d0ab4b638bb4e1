#!/usr/bin/env python3
"""Kernel time of frecsys_recommend against frecsys_eval_topk on the same
rows (loaded as the EVAL side, fold-in history excluded, k = 100): HIP-event
time of the library's own timers ("recommend", "eval_topk"), one warm-up, then
the median / min / max of 5 repetitions.

  a  all 116,677 rows x 20,108 items, d = 256 (the headline shape, random
     tables, the synthetic CSR bench.py builds for it)
  b  the first 64 rows of the same
  c  1,024 rows x 500,000 items, d = 1024 (random tables, 5..200 random
     history items per row)

Usage: recommend_bench.py [a|b|c ...] [--out FILE]
Prints one JSON line per case: times in ms, the item splits and row batches
chosen, and the scoring rate 2 rows items d / time in Tflop/s
(frecsys_work("recommend")).  The requirement read off case a: recommend's
median is not above eval_topk's median by more than eval_topk's spread
(max - min).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402
from frecsys_hip.data import SHAPES, synthetic  # noqa: E402

K, REPS = 100, 5


def _tables(rows, items, dim, seed):
    rng = np.random.default_rng(seed)
    s = dim ** -0.25
    X = rng.standard_normal((rows, dim), dtype=np.float32) * np.float32(s)
    V = rng.standard_normal((items, dim), dtype=np.float32) * np.float32(s)
    return X, V


def _timed(ctx, key, call):
    call()  # warm-up: allocations, code load
    ms, launches = [], 0
    for _ in range(REPS):
        ctx.timing_reset()
        call()
        t, launches = ctx.timing(key)
        ms.append(t)
    return ms, launches


def run_case(name, X, V, ep, ec):
    rows, dim = X.shape
    items = V.shape[0]
    ctx = fh.Context(dim, 1, items)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, ep, ec)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    out = {}
    rec, batches = _timed(ctx, "recommend", lambda: out.update(r=ctx.recommend(fh.SIDE_EVAL, K)))
    flops = ctx.work("recommend")[0]
    splits = ctx.counter("recommend_splits")
    top, _ = _timed(ctx, "eval_topk", lambda: out.update(t=ctx.eval_topk(K)))
    same = float(np.mean(np.all(out["r"][0] == out["t"], axis=1)))
    ctx.close()
    res = {
        "case": name, "rows": rows, "items": items, "dim": dim, "k": K,
        "recommend_ms": {"median": float(np.median(rec)), "min": min(rec), "max": max(rec)},
        "eval_topk_ms": {"median": float(np.median(top)), "min": min(top), "max": max(top)},
        "row_batches": batches,
        "splits": splits,
        "recommend_tflops": flops / (float(np.median(rec)) * 1e-3) / 1e12,
        "rows_identical_to_eval_topk": same,
    }
    res["slower_by_ms"] = res["recommend_ms"]["median"] - res["eval_topk_ms"]["median"]
    res["eval_topk_spread_ms"] = res["eval_topk_ms"]["max"] - res["eval_topk_ms"]["min"]
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    cases = args or ["a", "b", "c"]
    results = []
    if "a" in cases or "b" in cases:
        up, uc, ip, _ = synthetic(SHAPES["ml20m"])
        nu, ni = len(up) - 1, len(ip) - 1
        X, V = _tables(nu, ni, 256, 1)
        if "a" in cases:
            results.append(run_case("a", X, V, up, uc))
            print(json.dumps(results[-1]), flush=True)
        if "b" in cases:
            results.append(run_case("b", X[:64], V, up[:65], uc[:up[64]]))
            print(json.dumps(results[-1]), flush=True)
    if "c" in cases:
        rows, items, dim = 1024, 500_000, 1024
        X, V = _tables(rows, items, dim, 2)
        rng = np.random.default_rng(3)
        h = rng.integers(5, 201, rows)
        ep = np.concatenate([[0], np.cumsum(h)]).astype(np.int64)
        ec = rng.integers(0, items, int(ep[-1])).astype(np.int32)
        results.append(run_case("c", X, V, ep, ec))
        print(json.dumps(results[-1]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
