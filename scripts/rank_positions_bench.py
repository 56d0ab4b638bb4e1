#!/usr/bin/env python3
"""Kernel time of frecsys_rank_positions against the two ways the library had
before it of locating held-out items, on the same rows in the same process
(loaded as the EVAL side, fold-in history excluded, 10 random ground-truth
items per row; random N(0, d^-1/2) tables): HIP-event time of the library's own
timers, one warm-up, then the median / min / max of 5 repetitions.

  rank_positions  timer "rank_positions": history bits, prepare, scan, finish;
  recommend_1024  timer "recommend" of Context.recommend(k = 1024) -- the only
                  way to positions before, and only down to 1024 -- and the
                  host clock of the search of the ground truth in its lists;
  rank_metrics    timers "recommend" + "rank_metrics" of Context.rank_metrics
                  at the default cut-offs.

  a  all 116,677 rows x 20,108 items, d = 256 (the headline shape, random
     tables, the synthetic CSR bench.py builds for it)
  b  the first 64 rows of the same
  c  1,024 rows x 500,000 items, d = 1024 (random tables, 5..200 random
     history items per row)

Usage: rank_positions_bench.py [a|b|c ...] [--out FILE]
Prints one JSON line per case (--out appends them to FILE): times in ms, the
item splits and row batches chosen, the scoring rate 2 rows items d / time in
Tflop/s, and whether every rank below 1024 is the place in recommend's list.
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

GT, K, REPS = 10, 1024, 5


def _tables(rows, items, dim, seed):
    rng = np.random.default_rng(seed)
    s = dim ** -0.25
    X = rng.standard_normal((rows, dim), dtype=np.float32) * np.float32(s)
    V = rng.standard_normal((items, dim), dtype=np.float32) * np.float32(s)
    return X, V


def _stat(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def _timed(ctx, keys, call):
    call()  # warm-up: allocations, code load
    ms, launches = [], 0
    for _ in range(REPS):
        ctx.timing_reset()
        call()
        ms.append(sum(ctx.timing(k)[0] for k in keys))
        launches = ctx.timing(keys[0])[1]
    return ms, launches


def _host_search(items, gt):
    """Place of gt[i, j] in items[i], -1 when it is not listed."""
    out = np.full(gt.shape, -1, np.int32)
    for r0 in range(0, len(gt), 2048):
        hit = items[r0:r0 + 2048, :, None] == gt[r0:r0 + 2048, None, :]
        out[r0:r0 + 2048] = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)
    return out


def run_case(name, X, V, ep, ec):
    rows, dim = X.shape
    items = V.shape[0]
    rng = np.random.default_rng(11)
    gt = rng.integers(0, items, (rows, GT)).astype(np.int32)
    gp = (GT * np.arange(rows + 1)).astype(np.int64)
    ctx = fh.Context(dim, 1, items)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, ep, ec)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    out = {}
    pos, batches = _timed(ctx, ("rank_positions",), lambda: out.update(
        p=ctx.rank_positions(fh.SIDE_EVAL, gp, gt)))
    flops = ctx.work("rank_positions")[0]
    splits = ctx.counter("recommend_splits")
    rec, _ = _timed(ctx, ("recommend",), lambda: out.update(r=ctx.recommend(fh.SIDE_EVAL, K)))
    met, _ = _timed(ctx, ("recommend", "rank_metrics"), lambda: out.update(
        m=ctx.rank_metrics(fh.SIDE_EVAL, fh.EVAL_K_LIST, gp, gt)))
    ctx.close()
    host = []
    for i in range(3):
        t0 = time.perf_counter()
        place = _host_search(out["r"][0], gt)
        host.append((time.perf_counter() - t0) * 1e3)
    rank = out["p"][0].reshape(rows, GT)
    below = (rank >= 0) & (rank < K)
    res = {
        "case": name, "rows": rows, "items": items, "dim": dim, "ground_truth_per_row": GT,
        "rank_positions_ms": _stat(pos),
        "recommend_k1024_ms": _stat(rec),
        "host_search_ms": _stat(host),
        "rank_metrics_ms": _stat(met),
        "row_batches": batches,
        "splits": splits,
        "rank_positions_tflops": flops / (float(np.median(pos)) * 1e-3) / 1e12,
        "ranks_below_1024_equal_recommend": bool((np.where(below, rank, -1) == place).all()),
        "ranks_at_or_past_1024": float((rank >= K).mean()),
        "mean_mrr": float(out["p"][2].astype(np.float64).mean()),
        "mean_auc": float(out["p"][3].astype(np.float64).mean()),
    }
    res["faster_than_recommend_k1024_by_ms"] = (res["recommend_k1024_ms"]["median"] -
                                                res["rank_positions_ms"]["median"])
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    cases = args or ["a", "b", "c"]

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")

    if "a" in cases or "b" in cases:
        up, uc, ip, _ = synthetic(SHAPES["ml20m"])
        nu, ni = len(up) - 1, len(ip) - 1
        X, V = _tables(nu, ni, 256, 1)
        if "a" in cases:
            emit(run_case("a", X, V, up, uc))
        if "b" in cases:
            emit(run_case("b", X[:64], V, up[:65], uc[:up[64]]))
    if "c" in cases:
        rows, items, dim = 1024, 500_000, 1024
        X, V = _tables(rows, items, dim, 2)
        rng = np.random.default_rng(3)
        h = rng.integers(5, 201, rows)
        ep = np.concatenate([[0], np.cumsum(h)]).astype(np.int64)
        ec = rng.integers(0, items, int(ep[-1])).astype(np.int32)
        emit(run_case("c", X, V, ep, ec))


if __name__ == "__main__":
    main()
