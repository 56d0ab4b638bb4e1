#!/usr/bin/env python3
"""Kernel time of frecsys_recommend_dpp at the headline serving shape --
ML-20M-shaped item table (20,108 items), d = 256, 4,096 fold-in users, history
excluded -- for pool 200 / k 20 and pool 1024 / k 100, theta = 4, eps = 1e-3:
the two stages behind the scan ("diversify.gram", "dpp.select"), the scan in
front of them ("recommend") and the whole call (wall clock, copies included),
next to this build's frecsys_recommend_diverse (lam = 0.7) on the same rows in
the same session (its "diversify.gram" / "diversify.select": the yardstick),
to frecsys_recommend(k = pool) (the scan alone) and to a float64 numpy greedy
on a sample of rows (what the call replaces).  Where the factor fits LDS the
shape also runs with FRECSYS_DPP_FACTOR=ws (the factor in the workspace).
Library times are the HIP-event times of the library's own timers; one
warm-up, then the median / min / max of 5.

Usage: dpp_bench.py [--out FILE.jsonl] [--rows N]
Prints (and appends to FILE) one JSON line per shape and factor placement.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402

ITEMS, DIM, ROWS, REPS, THETA, EPS, LAM = 20_108, 256, 4096, 5, 4.0, 1e-3, 0.7
SHAPES = ((200, 20), (1024, 100))
NUMPY_SAMPLE = 16
LDS_BYTES = 40 * 1024  # kDppLdsBytes


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def _timed(ctx, keys, call):
    call()  # warm-up: allocations, code load
    ms = {k: [] for k in keys}
    wall = []
    for _ in range(REPS):
        ctx.timing_reset()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for k in keys:
            ms[k].append(ctx.timing(k)[0])
    return ms, wall


def _numpy_row(V64, ids, scores, k):
    """The greedy of include/frecsys_hip.h in float64, one row."""
    R = V64[ids]
    U = R / np.maximum(np.linalg.norm(R, axis=1, keepdims=True), 1e-300)
    S = U @ U.T
    rng = scores.max() - scores.min()
    w = np.exp2(THETA * ((scores - scores.min()) / rng if rng > 0 else np.zeros_like(scores)))
    r = np.ones(len(ids))
    alive = np.ones(len(ids), bool)
    C = np.zeros((k, len(ids)))
    out = []
    for t in range(k):
        E = alive & (r >= EPS)
        if not E.any():
            s = int(np.flatnonzero(alive)[0])
            out.append(ids[s])
            alive[s] = False
            continue
        s = int(np.argmax(np.where(E, w * r, -np.inf)))
        out.append(ids[s])
        alive[s] = False
        e = (S[s] - C[:t].T @ C[:t, s]) / np.sqrt(r[s])
        C[t] = e
        r = r - e * e
    return out


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

    ctx = fh.Context(DIM, 1, ITEMS)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, hp, hi)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    for pool, k in SHAPES:
        fits = 4 * k * pool <= LDS_BYTES
        for factor in (("lds", "ws") if fits else ("ws",)):
            os.environ.pop("FRECSYS_DPP_FACTOR", None)
            if fits and factor == "ws":
                os.environ["FRECSYS_DPP_FACTOR"] = "ws"
            out = {}
            keys = ("recommend", "diversify.gram", "dpp.select")
            dp, dp_wall = _timed(ctx, keys, lambda: out.update(
                d=ctx.recommend_dpp(fh.SIDE_EVAL, k, pool, THETA, EPS, return_gain=True)))
            flops, nbytes = ctx.work("dpp")[:2]
            subs = ctx.timing("dpp.select")[1]
            scan_batches = ctx.timing("recommend")[1]
            mkeys = ("recommend", "diversify.gram", "diversify.select")
            mm, mm_wall = _timed(ctx, mkeys, lambda: ctx.recommend_diverse(fh.SIDE_EVAL, k, pool, LAM))
            rec, rec_wall = _timed(ctx, ("recommend",), lambda: out.update(
                r=ctx.recommend(fh.SIDE_EVAL, pool)))
            lists, scores = out["r"]
            sample = np.linspace(0, rows - 1, NUMPY_SAMPLE).astype(int)
            t0 = time.perf_counter()
            ref = [_numpy_row(V64, lists[e], scores[e].astype(np.float64), k) for e in sample]
            np_ms = (time.perf_counter() - t0) * 1e3 / len(sample)
            agree = float(np.mean([np.mean(np.array(r) == out["d"][0][e])
                                   for e, r in zip(sample, ref)]))
            host = fh.dpp_select(V, lists[sample], scores[sample], k, THETA, EPS, return_gain=True)
            gram, sel = float(np.median(dp["diversify.gram"])), float(np.median(dp["dpp.select"]))
            scan = float(np.median(rec["recommend"]))
            res = {"bench": "dpp", "items": ITEMS, "dim": DIM, "rows": rows, "pool": pool, "k": k,
                   "theta": THETA, "eps": EPS, "factor": factor,
                   "gram_ms": _stats(dp["diversify.gram"]), "select_ms": _stats(dp["dpp.select"]),
                   "scan_in_call_ms": _stats(dp["recommend"]),
                   "recommend_dpp_wall_ms": _stats(dp_wall),
                   "mmr_gram_ms": _stats(mm["diversify.gram"]),
                   "mmr_select_ms": _stats(mm["diversify.select"]),
                   "recommend_diverse_wall_ms": _stats(mm_wall),
                   "recommend_k_pool_ms": _stats(rec["recommend"]),
                   "recommend_k_pool_wall_ms": _stats(rec_wall),
                   "scan_batches": scan_batches, "sub_batches": subs,
                   "dpp_steps_mean": float((out["d"][2] > 0).sum(1).mean()),
                   "added_over_scan": (gram + sel) / scan,
                   "select_over_mmr_select": sel / float(np.median(mm["diversify.select"])),
                   "dpp_us_per_row": (gram + sel) * 1e3 / rows,
                   "work_gflop": flops / 1e9, "work_gb": nbytes / 1e9,
                   "numpy_float64_us_per_row": np_ms * 1e3, "numpy_rows": len(sample),
                   "numpy_over_dpp": np_ms * 1e3 / ((gram + sel) * 1e3 / rows),
                   "positions_equal_to_numpy_float64": agree,
                   "identical_to_dpp_select": bool(
                       np.array_equal(host[0], out["d"][0][sample]) and
                       np.array_equal(host[2].view(np.uint32), out["d"][2][sample].view(np.uint32)))}
            line = json.dumps(res)
            print(line, flush=True)
            if out_path:
                os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
                with open(out_path, "a") as f:
                    f.write(line + "\n")
    os.environ.pop("FRECSYS_DPP_FACTOR", None)
    ctx.close()


if __name__ == "__main__":
    main()
