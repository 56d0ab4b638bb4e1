#!/usr/bin/env python3
"""Kernel time of frecsys_explain at the headline shape -- ML-20M-shaped item
table (20,108 items), iALS, d = 256 -- for 4,096 fold-in users x 10 targets x
top 10, next to the time frecsys_solve_side(EVAL) of the same build takes for
the same histories (explain repeats the solve's assembly and factorisation, so
the solve is its yardstick) and to the float64 numpy reference on a sample of
rows.  Library times are the HIP-event times of the library's own timers
("explain", "solve_eval"); one warm-up, then the median / min / max of 5.

Histories: log-normal lengths (median 68, mean ~ 140, clipped to [1, 4000],
ML-20M's shape), distinct random items.

Usage: explain_bench.py [--out FILE.jsonl] [--rows N]
Prints (and appends to FILE) one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402

ITEMS, DIM, ROWS, TARGETS, TOP, REPS = 20_108, 256, 4096, 10, 10, 5
REG, W = 0.003, 0.1
NUMPY_SAMPLE = 16


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def _timed(ctx, key, call):
    call()  # warm-up: allocations, code load
    ms = []
    for _ in range(REPS):
        ctx.timing_reset()
        call()
        ms.append(ctx.timing(key)[0])
    return ms


def _numpy_row(V, G, hist, targets):
    Y = V[hist].astype(np.float64)
    h = len(hist)
    lam = REG * (h + W * ITEMS)
    A = W * G + Y.T @ Y + lam * np.eye(DIM)
    Wt = np.linalg.solve(A, V[targets].astype(np.float64).T)
    c = Y @ Wt
    return c, c.sum(0)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else ROWS
    rng = np.random.default_rng(20)
    V = (rng.standard_normal((ITEMS, DIM), dtype=np.float32) * np.float32(DIM ** -0.5))
    lens = np.clip(np.exp(rng.normal(np.log(68.0), 1.2, rows)), 1, 4000).astype(np.int64)
    hp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hi = np.concatenate([rng.choice(ITEMS, h, replace=False) for h in lens]).astype(np.int32)
    tp = (TARGETS * np.arange(rows + 1)).astype(np.int64)
    tg = rng.integers(0, ITEMS, rows * TARGETS).astype(np.int32)

    ctx = fh.Context(DIM, 1, ITEMS)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, hp, hi)
    G = ctx.gramian(fh.SIDE_ITEM).astype(np.float64)
    out = {}
    ex = _timed(ctx, "explain", lambda: out.update(
        r=ctx.explain(fh.SIDE_EVAL, fh.KIND_IALS, REG, W, tp, tg, top=TOP)))
    flops, nbytes = ctx.work("explain")[:2]
    sv = _timed(ctx, "solve_eval", lambda: ctx.solve_side(fh.SIDE_EVAL, fh.KIND_IALS, REG, W))
    score = out["r"][0]
    ctx.close()

    sample = np.linspace(0, rows - 1, NUMPY_SAMPLE).astype(int)
    t0 = time.perf_counter()
    refs = [_numpy_row(V, G, hi[hp[e]:hp[e + 1]], tg[tp[e]:tp[e + 1]]) for e in sample]
    np_ms = (time.perf_counter() - t0) * 1e3 / len(sample)
    x_scale = max(float(np.abs(r[1]).max()) for r in refs)
    err = max(float(np.abs(score[tp[e]:tp[e + 1]] - r[1]).max()) for e, r in zip(sample, refs))

    ex_med, sv_med = float(np.median(ex)), float(np.median(sv))
    res = {"bench": "explain", "items": ITEMS, "dim": DIM, "rows": rows, "targets": TARGETS,
           "top": TOP, "mean_history": float(lens.mean()), "max_history": int(lens.max()),
           "explain_ms": _stats(ex), "solve_eval_ms": _stats(sv),
           "explain_us_per_row": ex_med * 1e3 / rows, "solve_us_per_row": sv_med * 1e3 / rows,
           "explain_over_solve": ex_med / sv_med,
           "numpy_float64_us_per_row": np_ms * 1e3, "numpy_rows": len(sample),
           "numpy_over_explain": np_ms * 1e3 / (ex_med * 1e3 / rows),
           "gflops": flops / (ex_med * 1e-3) / 1e9,
           "gather_gb_per_s": nbytes / (ex_med * 1e-3) / 1e9,
           "max_abs_score_diff_to_numpy": err, "max_abs_score": x_scale}
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
