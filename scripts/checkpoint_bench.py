#!/usr/bin/env python3
"""Save and load of a model checkpoint at a size a user runs: iALS, d = 256,
on the ML-20M shape bench.py's headline uses (the synthetic CSR it builds,
one Train() epoch so the tables are a trained model's).

Host clock around each call -- Model.save and Model.load return only after
their last device copy and (for save) the fsync and rename --, one warm-up,
then the median / min / max of 5 repetitions:

  save            Model.save(path): tables, state and the training tuples
  save_no_data    Model.save(path, include_data=False)
  load_resume     Model.load(path) of the first file: full verification, the
                  tuples from the file, both CSR orientations built and loaded
                  onto the device, tables set, Gramian rebuilt
  load_serve      Model.load(path) of the second file (no tuples, no CSR)
  file_info       fh.model_file_info(path, verify=True) of the first file:
                  the host-only verification pass load starts with

Usage: checkpoint_bench.py [--dir DIR] [--out FILE]
DIR (default: a fresh temporary directory) decides which file system is
measured; it is reported.  Prints one JSON line per measurement (--out appends
them to FILE): file bytes, seconds and GB/s (file bytes / seconds).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402
from frecsys_hip.data import SHAPES, synthetic  # noqa: E402

REPS = 5
DIM = 256


def _timed(call, after=None):
    out = []
    for rep in range(REPS + 1):  # the first one is the warm-up
        t0 = time.perf_counter()
        r = call()
        dt = time.perf_counter() - t0
        if after:
            after(r)
        if rep:
            out.append(dt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if fh.device_count() < 1:
        sys.exit("checkpoint_bench.py needs a GPU")
    work = args.dir or tempfile.mkdtemp(prefix="frecsys_ckpt_")
    os.makedirs(work, exist_ok=True)
    full, bare = os.path.join(work, "bench.frecsys"), os.path.join(work, "bench_nodata.frecsys")

    up, uc, ip, ic = synthetic(SHAPES["ml20m"])
    nu, ni = len(up) - 1, len(ip) - 1
    users = np.repeat(np.arange(nu, dtype=np.int32), np.diff(up))
    items = np.asarray(uc, dtype=np.int32)
    m = fh.Model("ials", users, items, dim=DIM, seed=1, stdev=0.1, l2_reg=0.003, uobs_weight=0.1,
                 print_train_stats=False)
    m.train(1)
    m.context().synchronize()

    lines = []

    def report(what, path, secs):
        size = os.path.getsize(path)
        med = float(np.median(secs))
        lines.append({"what": what, "model": "ials", "dim": DIM, "n_users": nu, "n_items": ni,
                      "n_tuples": int(len(users)), "file_bytes": size, "reps": REPS,
                      "seconds_median": med, "seconds_min": float(min(secs)),
                      "seconds_max": float(max(secs)), "gb_per_s": size / med / 1e9,
                      "dir": work})
        print(json.dumps(lines[-1]), flush=True)

    report("save", full, _timed(lambda: m.save(full)))
    report("save_no_data", bare, _timed(lambda: m.save(bare, include_data=False)))
    m.close()
    report("file_info", full, _timed(lambda: fh.model_file_info(full, verify=True)))
    report("load_resume", full, _timed(lambda: fh.Model.load(full), after=lambda x: x.close()))
    report("load_serve", bare, _timed(lambda: fh.Model.load(bare), after=lambda x: x.close()))
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if not args.dir:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
