#!/usr/bin/env python3
"""Kernel time of frecsys_similar, dot against cosine, on the two tables of
the headline (ML-20M) shape at d = 256, k = 10: HIP-event time of the
library's own timers ("similar", "similar.norms"), one warm-up, then the
median / min / max of 5 repetitions, all in one process.

  items  20,108 x 256, every item a query
  users  116,677 x 256, 4,096 queries (a fixed random subset)

Usage: similar_bench.py [items|users ...] [--out FILE]
Prints one JSON line per case and metric: times in ms, the row batches, the
scoring rate 2 queries rows d / time in Tflop/s (frecsys_work("similar")), the
norm pass's share of the cosine call, and cosine's excess over dot next to the
dot runs' own spread.  The dot call with keep_self runs frecsys_recommend's own
scan instantiation; it is timed too, as the yardstick of the variant.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402
from frecsys_hip.data import SHAPES  # noqa: E402

K, REPS, DIM = 10, 5, 256


def _timed(ctx, call):
    call()  # warm-up: allocations, code load
    scan, norms, launches = [], [], 0
    for _ in range(REPS):
        ctx.timing_reset()
        call()
        t, launches = ctx.timing("similar")
        scan.append(t)
        norms.append(ctx.timing("similar.norms")[0])
    return scan, norms, launches


def _stats(ms):
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms)}


def run_case(name, m, queries):
    rng = np.random.default_rng(4)
    T = rng.standard_normal((m, DIM), dtype=np.float32) * np.float32(DIM ** -0.25)
    # norms spread over a decade, so that the two rankings differ
    T *= (10.0 ** rng.uniform(-0.5, 0.5, (m, 1))).astype(np.float32)
    rows = None if queries is None else np.sort(rng.permutation(m)[:queries]).astype(np.int64)
    n = m if rows is None else len(rows)
    user = name == "users"
    side = fh.SIDE_USER if user else fh.SIDE_ITEM
    ctx = fh.Context(DIM, m if user else 1, 1 if user else m)
    ctx.set_embeddings(side, T)
    res = []
    runs = {}
    for label, cosine, keep in (("dot_keep_self", False, True), ("dot", False, False),
                                ("cosine", True, False)):
        scan, norms, batches = _timed(
            ctx, lambda: ctx.similar(side, K, rows=rows, cosine=cosine, keep_self=keep))
        flops, nbytes = ctx.work("similar")[:2]   # of the last call: timing_reset clears it
        total = [s + t for s, t in zip(scan, norms)]
        runs[label] = total
        r = {"case": name, "metric": label, "rows": m, "queries": n, "dim": DIM, "k": K,
             "scan_ms": _stats(scan), "norms_ms": _stats(norms), "total_ms": _stats(total),
             "row_batches": batches, "flops": flops, "bytes": nbytes,
             "tflops": flops / (float(np.median(total)) * 1e-3) / 1e12,
             "norms_share": float(np.median(norms)) / float(np.median(total))}
        res.append(r)
    dot, cos = runs["dot"], runs["cosine"]
    res[-1]["cosine_over_dot_ms"] = float(np.median(cos)) - float(np.median(dot))
    res[-1]["dot_spread_ms"] = max(dot) - min(dot)
    ctx.close()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    cases = args or ["items", "users"]
    shape = SHAPES["ml20m"]
    lines = []
    for name in cases:
        m = {"items": shape.n_items, "users": shape.n_users}[name]
        for r in run_case(name, m, None if name == "items" else 4096):
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
