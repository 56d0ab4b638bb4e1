#!/usr/bin/env python3
"""Kernel time of frecsys_recommend_two_stage against frecsys_recommend on
the same rows in the same process, alternating: HIP-event time of the library's
own timers, one warm-up, then the median [min, max] of 5 repetitions.

  a, b, c   the cases of scripts/recommend_bench.py (random tables, the same
            CSR, k = 100, history excluded)
  ml20m     iALS at d = 256 trained for 3 epochs on the ML-20M-shaped
            synthetic data, every user
  ml1m      iALS at d = 64 trained for 3 epochs on tests/golden/ml-1m

Per case the pool is swept over {2 k, 4 k, 1024} with the fallback off and on.
One JSON line per run: the four two-stage timer keys and their sum, the exact
call's time, the certified share, the fallback rows, and the scan's rate
against the bf16 matrix peak (2.5 Pflop/s) and its booked bytes against the
measured HBM rate (6.2 TB/s) -- `bound` names the larger of the two shares,
or "neither" when both are below a tenth.

Usage: two_stage_bench.py [a|b|c|ml20m|ml1m ...] [--out FILE]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402
from frecsys_hip.data import SHAPES, Dataset, synthetic  # noqa: E402

K, REPS = 100, 5
KEYS = ("two_stage.convert", "two_stage.scan", "two_stage.select", "two_stage.fallback")
BF16_PEAK, HBM_RATE = 2.5e15, 6.2e12


def _tables(rows, items, dim, seed):
    rng = np.random.default_rng(seed)
    s = dim ** -0.25
    X = rng.standard_normal((rows, dim), dtype=np.float32) * np.float32(s)
    V = rng.standard_normal((items, dim), dtype=np.float32) * np.float32(s)
    return X, V


def _stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def sweep(name, ctx, side, rows, items, dim, k, emit):
    """Both calls on every row of `side`, alternating, for every pool and mode."""
    for pool in sorted({min(1024, 2 * k), min(1024, 4 * k), 1024}):
        for exact in (False, True):
            out = {}

            def exact_call():
                out["r"] = ctx.recommend(side, k)

            def two_call():
                out["t"] = ctx.recommend_two_stage(side, k, pool, exact=exact)
            exact_call()
            two_call()  # warm-up: allocations, code load
            rec, two = [], {key: [] for key in KEYS}
            fb0 = ctx.counter("two_stage_fallback_rows")
            for _ in range(REPS):
                ctx.timing_reset()
                exact_call()
                rec.append(ctx.timing("recommend")[0])
                ctx.timing_reset()
                two_call()
                for key in KEYS:
                    two[key].append(ctx.timing(key)[0])
            total = [sum(two[key][i] for key in KEYS) for i in range(REPS)]
            cert = out["t"][2]
            dh = max(16, ctx.lib.frecsys_padded_dim(dim))
            scan_s = float(np.median(two["two_stage.scan"])) * 1e-3
            flops = 2.0 * rows * items * dim
            nbytes = (rows + items) * dh * 2.0 + 8.0 * rows * pool
            mfma, mem = flops / scan_s / BF16_PEAK, nbytes / scan_s / HBM_RATE
            same = float(np.mean(np.all(out["t"][0] == out["r"][0], axis=1)))
            bound = "neither" if max(mfma, mem) < 0.1 else ("matrix" if mfma > mem else "memory")
            emit({"case": name, "rows": rows, "items": items, "dim": dim, "k": k, "pool": pool,
                  "exact": exact, "recommend_ms": _stat(rec), "two_stage_ms": _stat(total),
                  **{key.replace("two_stage.", "") + "_ms": _stat(two[key]) for key in KEYS},
                  "speedup": float(np.median(rec)) / float(np.median(total)),
                  "certified_share": float(np.mean(cert == 1)),
                  "fallback_rows": (ctx.counter("two_stage_fallback_rows") - fb0) // REPS,
                  "rows_identical_to_recommend": same,
                  "scan_tflops": flops / scan_s / 1e12, "scan_share_of_bf16_peak": mfma,
                  "scan_share_of_hbm_rate": mem, "bound": bound})


def random_case(name, X, V, ep, ec, emit):
    rows, dim = X.shape
    ctx = fh.Context(dim, 1, V.shape[0])
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, ep, ec)
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    sweep(name, ctx, fh.SIDE_EVAL, rows, V.shape[0], dim, K, emit)
    ctx.close()


def trained_case(name, users, items, dim, emit):
    m = fh.Model("ials", users, items, dim=dim, stdev=0.1, seed=1, l2_reg=0.003, l2_reg_exp=1.0,
                 uobs_weight=0.1, print_train_stats=False)
    m.initialize()
    m.train(3)
    sweep(name, m.context(), fh.SIDE_USER, m.n_users, m.n_items, dim, K, emit)
    m.close()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    cases = args or ["a", "b", "c", "ml20m", "ml1m"]
    sink = open(out_path, "a") if out_path else None

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    if {"a", "b", "ml20m"} & set(cases):
        up, uc, ip, _ = synthetic(SHAPES["ml20m"])
        nu, ni = len(up) - 1, len(ip) - 1
        if {"a", "b"} & set(cases):
            X, V = _tables(nu, ni, 256, 1)
            if "a" in cases:
                random_case("a", X, V, up, uc, emit)
            if "b" in cases:
                random_case("b", X[:64], V, up[:65], uc[:up[64]], emit)
        if "ml20m" in cases:
            trained_case("ml20m", np.repeat(np.arange(nu, dtype=np.int32), np.diff(up)),
                         np.asarray(uc, np.int32), 256, emit)
    if "c" in cases:
        rows, items, dim = 1024, 500_000, 1024
        X, V = _tables(rows, items, dim, 2)
        rng = np.random.default_rng(3)
        h = rng.integers(5, 201, rows)
        ep = np.concatenate([[0], np.cumsum(h)]).astype(np.int64)
        ec = rng.integers(0, items, int(ep[-1])).astype(np.int32)
        random_case("c", X, V, ep, ec, emit)
    if "ml1m" in cases:
        tr = Dataset.from_csv(os.path.join(ROOT, "tests", "golden", "ml-1m", "train.csv"))
        trained_case("ml1m", tr.users, tr.items, 64, emit)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
