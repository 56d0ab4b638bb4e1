#!/usr/bin/env python3
"""One iALS Train() epoch at d = 256 on the ML-20M shape (the headline
workload of bench.py, its flags): the LLT path against --use_cg, on one
build, in one process.

  llt            the direct solve (the comparison line)
  cg3 / cg10     use_cg, cg_max_iterations 3 / 10, tolerance 1e-10
  cg100          use_cg, cap 100, tolerance 1e-10
  cg100_tol1e-3  use_cg, cap 100, tolerance 1e-3

Per configuration: a fresh model from seed 1, WARMUP epochs, then STEPS timed
epochs (a host clock around model.train(1) + a device synchronise), reported
as median / min / max, with the library's own HIP-event timers per epoch,
and for the CG runs the iterations per epoch (counter "cg_iterations"), the
entities that stopped at the cap, and the achieved rate of the CG kernels:
frecsys_work("<solve>.cg") gather bytes and flops over their event time.

Usage: cg_bench.py [config ...] [--steps N] [--warmup N] [--dim D] [--shape S] [--out FILE]
Prints one JSON line per configuration.
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

FLAGS = dict(l2_reg=0.003, uobs_weight=0.1, l2_reg_exp=1.0)  # bench.py ials_ml20m_d256
CONFIGS = {
    "llt": dict(use_cg=False),
    "cg3": dict(use_cg=True, cg_max_iterations=3, cg_error_tolerance=1e-10),
    "cg10": dict(use_cg=True, cg_max_iterations=10, cg_error_tolerance=1e-10),
    "cg100": dict(use_cg=True, cg_max_iterations=100, cg_error_tolerance=1e-10),
    "cg100_tol1e-3": dict(use_cg=True, cg_max_iterations=100, cg_error_tolerance=1e-3),
}
SIDES = ("solve_user", "solve_item")


def _opt(name, default):
    if name in sys.argv:
        return sys.argv[sys.argv.index(name) + 1]
    return default


def run_config(name, users, items, dim, steps, warmup):
    model = fh.Model("ials", users, items, dim=dim, stdev=0.1, seed=1, print_train_stats=False,
                     device=0, **FLAGS, **CONFIGS[name])
    ctx = model.context()
    model.train(warmup)
    ctx.synchronize()
    wall, per = [], []
    it0, un0 = ctx.counter("cg_iterations"), ctx.counter("cg_unconverged")
    for _ in range(steps):
        ctx.timing_reset()
        t0 = time.perf_counter()
        model.train(1)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ep = {k: ctx.timing(k)[0] for k in SIDES + ("gramian", "user_loss")}
        for s in SIDES:
            ms = ctx.timing(s + ".cg")[0]
            fl, by, ne, _ = ctx.work(s + ".cg")
            ep[s + ".cg"] = ms
            ep[s + ".cg_flops"], ep[s + ".cg_bytes"], ep[s + ".cg_entities"] = fl, by, ne
        it1, un1 = ctx.counter("cg_iterations"), ctx.counter("cg_unconverged")
        ep["cg_iterations"], ep["cg_unconverged"] = it1 - it0, un1 - un0
        it0, un0 = it1, un1
        per.append(ep)
    res = {"config": name, "model": "ials", "dim": dim, "flags": {**FLAGS, **CONFIGS[name]},
           "steps": steps, "warmup": warmup,
           "epoch_ms": {"median": float(np.median(wall)), "min": min(wall), "max": max(wall),
                        "all": wall},
           "kernel_ms_per_epoch": {k: float(np.median([e[k] for e in per]))
                                   for k in SIDES + ("gramian", "user_loss")}}
    if CONFIGS[name]["use_cg"]:
        res["cg_iterations_per_epoch"] = [e["cg_iterations"] for e in per]
        res["cg_unconverged_per_epoch"] = [e["cg_unconverged"] for e in per]
        for s in SIDES:
            ms = float(np.median([e[s + ".cg"] for e in per]))
            by = float(np.median([e[s + ".cg_bytes"] for e in per]))
            fl = float(np.median([e[s + ".cg_flops"] for e in per]))
            ne = per[-1][s + ".cg_entities"]
            res[s + ".cg"] = {
                "ms": ms, "entities": ne,
                "gather_GBps": by / (ms * 1e-3) / 1e9 if ms > 0 else None,
                "gflops": fl / (ms * 1e-3) / 1e9 if ms > 0 else None}
    ctx.close()
    model.close()
    return res


def main():
    steps, warmup = int(_opt("--steps", 3)), int(_opt("--warmup", 1))
    dim, shape = int(_opt("--dim", 256)), _opt("--shape", "ml20m")
    out_path = _opt("--out", None)
    skip = set()
    for flag in ("--steps", "--warmup", "--dim", "--shape", "--out"):
        if flag in sys.argv:
            skip |= {sys.argv.index(flag), sys.argv.index(flag) + 1}
    names = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip] or list(CONFIGS)
    up, uc, _, _ = synthetic(SHAPES[shape])
    users = np.repeat(np.arange(len(up) - 1, dtype=np.int32), np.diff(up))
    results = []
    for name in names:
        results.append(run_config(name, users, uc, dim, steps, warmup))
        print(json.dumps(results[-1]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
