#!/usr/bin/env python3
"""Kernel time of frecsys_rank_quality at the headline serving shape --
ML-20M-shaped item table (20,108 items), d = 256, 4,096 fold-in users, history
excluded, cut-offs 5 / 10 / 20, novelty weights and a ground truth given -- for
the plain top-20 (pool 0) and for pool 200 / lam 0.7: the two added stages
("quality", "quality.exposure") beside the scan ("recommend"), the MMR stages
("diversify.gram", "diversify.select") and the metrics kernel ("rank_metrics")
of the same call, the whole call (wall clock, copies included), and a float64
numpy computation of the same numbers on the fetched lists (what the call
replaces; a sample of rows, per row).  Library times are the HIP-event times of
the library's own timers; one warm-up, then the median / min / max of 5.

Then the curve the call exists for: Recall@20 / NDCG@20 / ILD@20 / coverage@20
/ Gini@20 over lam in {1, 0.9, 0.7, 0.5, 0.3} at pool 200, on tables of the same
shape with structure for lam to act on (items in 64 clusters, users near two
centres each; Gaussian rows at d = 256 are nearly orthogonal).  The tables are
synthetic, so the ground truth is too: ten items drawn from each user's own
top 50 (history excluded), which makes Recall fall as lam moves the lists away
from the plain ranking.

Usage: quality_bench.py [--out FILE.jsonl] [--rows N]
Prints (and appends to FILE) one JSON line per configuration and per lam.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402

ITEMS, DIM, ROWS, REPS = 20_108, 256, 4096, 5
KS = (5, 10, 20)
CONFIGS = ((None, 1.0), (200, 0.7))
LAMS = (1.0, 0.9, 0.7, 0.5, 0.3)
NUMPY_SAMPLE = 256
KEYS = ("recommend", "diversify.gram", "diversify.select", "rank_metrics", "quality",
        "quality.exposure")


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def _timed(ctx, call):
    call()  # warm-up: allocations, code load
    ms = {k: [] for k in KEYS}
    wall = []
    for _ in range(REPS):
        ctx.timing_reset()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for k in KEYS:
            ms[k].append(ctx.timing(k)[0])
    return ms, wall


def _numpy_quality(V64, lists, w64):
    """ILD, novelty and exposure per cut-off in float64, pairwise."""
    ild = np.zeros((len(lists), len(KS)))
    nov = np.zeros_like(ild)
    exposure = np.zeros((len(KS), len(V64)), np.int64)
    for i, row in enumerate(lists):
        for q, K in enumerate(KS):
            ids = row[:K][row[:K] >= 0]
            R = V64[ids]
            R = R / np.maximum(np.linalg.norm(R, axis=1, keepdims=True), 1e-300)
            n = len(ids)
            if n >= 2:
                ild[i, q] = 1.0 - np.triu(R @ R.T, 1).sum() / (n * (n - 1) // 2)
            if n >= 1:
                nov[i, q] = w64[ids].sum() / n
            exposure[q] += np.bincount(ids, minlength=len(V64))
    return ild, nov, exposure


def _emit(res, out_path):
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else ROWS
    rng = np.random.default_rng(30)
    s = np.float32(DIM ** -0.25)
    V = rng.standard_normal((ITEMS, DIM), dtype=np.float32) * s
    X = rng.standard_normal((rows, DIM), dtype=np.float32) * s
    lens = np.clip(np.exp(rng.normal(np.log(68.0), 1.2, rows)), 1, 4000).astype(np.int64)
    hp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hi = np.concatenate([rng.choice(ITEMS, h, replace=False) for h in lens]).astype(np.int32)
    V64 = V.astype(np.float64)
    # self information of the items by their share of the histories
    w = (-np.log2(np.maximum(np.bincount(hi, minlength=ITEMS), 1) / rows)).astype(np.float32)
    w64 = w.astype(np.float64)

    ctx = fh.Context(DIM, 1, ITEMS)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, hp, hi)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    top50 = ctx.recommend(fh.SIDE_EVAL, 50)[0]
    gi = np.concatenate([rng.choice(r, 10, replace=False) for r in top50]).astype(np.int32)
    gp = (10 * np.arange(rows + 1)).astype(np.int64)

    sample = np.linspace(0, rows - 1, min(rows, NUMPY_SAMPLE)).astype(int)
    for pool, lam in CONFIGS:
        out = {}
        ms, wall = _timed(ctx, lambda: out.update(q=ctx.rank_quality(
            fh.SIDE_EVAL, KS, pool=pool, lam=lam, item_weight=w, gt=(gp, gi))))
        flops, nbytes = ctx.work("quality")[:2]
        batches = ctx.timing("recommend")[1]
        if pool is None:
            lists = ctx.recommend(fh.SIDE_EVAL, max(KS))[0]
        else:
            lists = ctx.recommend_diverse(fh.SIDE_EVAL, max(KS), pool, lam)[0]
        t0 = time.perf_counter()
        ref = _numpy_quality(V64, lists[sample], w64)
        np_us = (time.perf_counter() - t0) * 1e6 / len(sample)
        got = out["q"]
        err = max(float(np.max(np.abs(got[k][sample].astype(np.float64) - r) /
                               np.maximum(1.0, np.abs(r)))) for k, r in
                  (("ild", ref[0]), ("novelty", ref[1])))
        host = fh.list_quality(V, lists, KS, w)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        added = med["quality"] + med["quality.exposure"]
        _emit({"bench": "quality", "items": ITEMS, "dim": DIM, "rows": rows, "k_list": KS,
               "pool": pool or 0, "lam": lam, "scan_batches": batches,
               **{k.replace(".", "_") + "_ms": _stats(v) for k, v in ms.items()},
               "rank_quality_wall_ms": _stats(wall),
               "added_over_scan": added / med["recommend"],
               "quality_over_scan": med["quality"] / med["recommend"],
               "quality_us_per_row": med["quality"] * 1e3 / rows,
               "quality_gb_per_s": nbytes / (med["quality"] * 1e-3) / 1e9,
               "work_gflop": flops / 1e9, "work_gb": nbytes / 1e9,
               "numpy_float64_us_per_row": np_us, "numpy_rows": len(sample),
               "numpy_over_added": np_us / (added * 1e3 / rows),
               "max_err_vs_numpy_over_2^-23": err / 2.0 ** -23,
               "exposure_equal_to_host": bool(np.array_equal(got["exposure"], host[2])),
               "max_err_vs_host_over_2^-23": float(np.max(
                   np.abs(got["ild"].astype(np.float64) - host[0]) /
                   np.maximum(1.0, np.abs(host[0])))) / 2.0 ** -23}, out_path)

    # the curve: Gaussian rows at d = 256 are nearly orthogonal, so there is no
    # similarity for lam to trade; items in 64 clusters (a centre plus noise,
    # cosine about 0.64 within a cluster) and users near two centres each
    centres = rng.standard_normal((64, DIM), dtype=np.float32)
    V = (0.8 * centres[rng.integers(0, 64, ITEMS)] +
         0.6 * rng.standard_normal((ITEMS, DIM), dtype=np.float32)) * s
    X = (centres[rng.integers(0, 64, rows)] + centres[rng.integers(0, 64, rows)] +
         0.5 * rng.standard_normal((rows, DIM), dtype=np.float32)) * s
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    top50 = ctx.recommend(fh.SIDE_EVAL, 50)[0]
    gi = np.concatenate([rng.choice(r, 10, replace=False) for r in top50]).astype(np.int32)
    q20 = KS.index(20)
    for lam in LAMS:
        got = ctx.rank_quality(fh.SIDE_EVAL, KS, pool=200, lam=lam, item_weight=w, gt=(gp, gi))
        summ = fh.exposure_summary(got["exposure"][q20])
        _emit({"bench": "quality_curve", "items": ITEMS, "dim": DIM, "rows": rows, "pool": 200,
               "k": 20, "tables": "64 clusters", "lam": lam, "recall": float(got["recall"][:, q20].mean(dtype=np.float64)),
               "ndcg": float(got["ndcg"][:, q20].mean(dtype=np.float64)),
               "ild": float(got["ild"][:, q20].mean(dtype=np.float64)),
               "novelty": float(got["novelty"][:, q20].mean(dtype=np.float64)),
               "coverage": summ["coverage"], "gini": summ["gini"]}, out_path)
    ctx.close()


if __name__ == "__main__":
    main()
