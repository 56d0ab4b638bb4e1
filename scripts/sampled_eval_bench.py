#!/usr/bin/env python3
"""Sampled evaluation on the device (Context.sampled_metrics) against what a
caller composes without it: negatives drawn on the host with
fh.sample_negatives (the same generator, so the lists are identical), the
lists built in numpy, Context.rank_candidates, fh.list_metrics.  Both sides
are timed end to end on the host clock; the fused call also reports the HIP
event time of its timer keys ("sample_negatives", "rank_candidates",
"rank_metrics").  One warm-up, then the median / min / max of 5.

  a  116,677 users x 20,108 items, d = 256 (the synthetic ML-20M CSR of
     bench.py), the last 5 items of every history held out as ground truth,
     n_neg = 1000, the default cut-offs, the remaining history excluded; also
     the full-catalogue Context.rank_metrics (what Model.evaluate runs) on
     the same rows, reported only
  b  100,000 fold-in rows (EVAL side, 20-item histories, 5 held-out items) x
     500,000 items, d = 1024, n_neg = 1000

Usage: sampled_eval_bench.py [a|b ...] [--out FILE.jsonl]
Prints (and appends to FILE) one JSON line per case.  The bar: the fused
call's median below the yardstick's median, and its max below the yardstick's
min.  The tables are random (timing does not depend on their values).
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

K_LIST, N_NEG, SEED, REPS, HELD = fh.EVAL_K_LIST, 1000, 20260, 5, 5
KEYS = ("sample_negatives", "rank_candidates", "rank_metrics")


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def _tables(rows, items, dim, seed):
    rng = np.random.default_rng(seed)
    s = np.float32(dim ** -0.25)
    return (rng.standard_normal((rows, dim), dtype=np.float32) * s,
            rng.standard_normal((items, dim), dtype=np.float32) * s)


def _hold_out(ptr, col):
    """The last HELD items of every row as ground truth, the rest as history
    (a row of exactly HELD items keeps an empty history)."""
    n = len(ptr) - 1
    lens = np.diff(ptr)
    assert lens.min() >= HELD
    pos = np.arange(ptr[-1]) - np.repeat(ptr[:-1], lens)
    held = pos >= np.repeat(lens - HELD, lens)
    gp = (HELD * np.arange(n + 1)).astype(np.int64)
    hp = np.concatenate([[0], np.cumsum(lens - HELD)]).astype(np.int64)
    return hp, col[~held].astype(np.int32), gp, col[held].astype(np.int32)


def _lists(n_items, hp, hc, gp, gi, cnt, neg):
    """The candidate lists of the sampler's outputs: ground truth (distinct
    here), then the negatives -- the whole pool for a whole-pool row."""
    n = len(gp) - 1
    whole = np.nonzero((cnt != N_NEG) | (neg[:, 0] == -1))[0]
    if len(whole) == 0:
        ci = np.concatenate([gi.reshape(n, HELD), neg], axis=1).reshape(-1)
        return ((HELD + N_NEG) * np.arange(n + 1)).astype(np.int64), ci
    out = []
    for i in range(n):
        g = gi[gp[i]:gp[i + 1]]
        if cnt[i] != N_NEG or neg[i, 0] == -1:
            ok = np.ones(n_items, bool)
            ok[g] = False
            ok[hc[hp[i]:hp[i + 1]]] = False
            out.append(np.concatenate([g, np.nonzero(ok)[0].astype(np.int32)]))
        else:
            out.append(np.concatenate([g, neg[i]]))
    cp = np.concatenate([[0], np.cumsum([len(c) for c in out])]).astype(np.int64)
    return cp, np.concatenate(out).astype(np.int32)


def _timed(call):
    call()   # warm-up: allocations, code load
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def run(name, side, ctx, n, n_items, dim, hp, hc, gp, gi, full=False):
    out = {}

    def fused():
        out["f"] = ctx.sampled_metrics(side, K_LIST, gp, gi, N_NEG, SEED)

    def composed():
        cnt, neg = fh.sample_negatives(n_items, gp, gi, N_NEG, SEED, hist_ptr=hp, hist_items=hc)
        cp, ci = _lists(n_items, hp, hc, gp, gi, cnt, neg)
        items, _ = ctx.rank_candidates(side, max(K_LIST), cp, ci)
        out["c"] = fh.list_metrics(items, gp, gi, K_LIST)
        out["whole"] = int(((cnt != N_NEG) | (neg[:, 0] == -1)).sum())

    fused()
    dev = {}
    fus = []
    for _ in range(REPS):
        ctx.timing_reset()
        t0 = time.perf_counter()
        fused()
        fus.append((time.perf_counter() - t0) * 1e3)
        for key in KEYS:
            dev.setdefault(key, []).append(ctx.timing(key)[0])
    launches = {key: ctx.timing(key)[1] for key in KEYS}
    work = {key: ctx.work(key)[1] for key in KEYS}
    com = _timed(composed)
    same = bool(np.array_equal(out["f"][0].view(np.uint32), out["c"][0].view(np.uint32)) and
                np.array_equal(out["f"][1].view(np.uint32), out["c"][1].view(np.uint32)))
    res = {"case": name, "rows": n, "items": n_items, "dim": dim, "n_neg": N_NEG,
           "k_list": list(K_LIST), "whole_pool_rows": out["whole"],
           "fused_host_ms": _stats(fus), "composed_host_ms": _stats(com),
           "fused_device_ms": {key: _stats(dev[key]) for key in KEYS},
           "launches": launches, "bitwise_equal_to_composed": same,
           "mean_recall": [float(x) for x in out["f"][0].mean(axis=0)]}
    s, r = np.median(dev["sample_negatives"]), np.median(dev["rank_candidates"])
    res["sample_share_of_device"] = float(s / (s + r + np.median(dev["rank_metrics"])))
    res["sample_over_rank"] = float(s / r)
    res["rank_candidates_tb_per_s"] = float(work["rank_candidates"] / (r * 1e-3) / 1e12)
    res["sample_negatives_tb_per_s"] = float(work["sample_negatives"] / (s * 1e-3) / 1e12)
    f, c = res["fused_host_ms"], res["composed_host_ms"]
    res["median_below"] = bool(f["median"] < c["median"])
    res["max_below_min"] = bool(f["max"] < c["min"])
    res["bar_met"] = res["median_below"] and res["max_below_min"]
    res["speedup_median"] = c["median"] / f["median"]
    if full:
        ms = _timed(lambda: out.update(full=ctx.rank_metrics(side, K_LIST, gp, gi)))
        res["full_catalogue_rank_metrics_host_ms"] = _stats(ms)
        res["full_over_fused_median"] = float(np.median(ms)) / f["median"]
        res["full_mean_recall"] = [float(x) for x in out["full"][0].mean(axis=0)]
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    cases = args or ["a", "b"]

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(line + "\n")

    if "a" in cases:
        up, uc = synthetic(SHAPES["ml20m"])[:2]
        n, n_items, dim = len(up) - 1, SHAPES["ml20m"].n_items, 256
        hp, hc, gp, gi = _hold_out(up, uc)
        X, V = _tables(n, n_items, dim, 1)
        with fh.Context(dim, n, n_items) as ctx:
            ctx.load_csr(fh.SIDE_USER, hp, hc)
            ctx.set_embeddings(fh.SIDE_USER, X)
            ctx.set_embeddings(fh.SIDE_ITEM, V)
            emit(run("a", fh.SIDE_USER, ctx, n, n_items, dim, hp, hc, gp, gi, full=True))
    if "b" in cases:
        n, n_items, dim, hist = 100_000, 500_000, 1024, 20
        rng = np.random.default_rng(3)
        # distinct per row: a random start and a stride that is odd (no wrap within 25 steps)
        start = rng.integers(0, n_items, n)[:, None]
        step = (2 * rng.integers(1, 5000, n) + 1)[:, None]
        ids = ((start + step * np.arange(hist + HELD)[None, :]) % n_items).astype(np.int32)
        ptr = ((hist + HELD) * np.arange(n + 1)).astype(np.int64)
        hp, hc, gp, gi = _hold_out(ptr, ids.reshape(-1))
        X, V = _tables(n, n_items, dim, 2)
        with fh.Context(dim, 1, n_items) as ctx:
            ctx.set_embeddings(fh.SIDE_ITEM, V)
            ctx.load_csr(fh.SIDE_EVAL, hp, hc)
            ctx.set_embeddings(fh.SIDE_EVAL, X)
            emit(run("b", fh.SIDE_EVAL, ctx, n, n_items, dim, hp, hc, gp, gi))


if __name__ == "__main__":
    main()
