#!/usr/bin/env python3
"""Kernel time of frecsys_audience on the headline (ML-20M) shape at d = 256:
n query items of a 20,108-row item table against the 116,677-row user table,
the thin-query kernel (FRECSYS_AUDIENCE_THIN_MAX forced high) against the scan
path (forced 0), and against the yardstick a build without the call has:
Context.similar(SIDE_USER, k, rows=<n ids>, cosine=False, keep_self=True), the
same scan kernel over the same table with the same n and k.  HIP-event time of
the library's own timers ("audience", "similar"), one warm-up, then the median /
min / max of 5 repetitions, all in one process.

Usage: audience_bench.py [main|sweep|exclude|big|yardstick ...] [--label NAME]
                         [--pkg DIR] [--out FILE]
  main       n in {1, 8, 64, 1024} x k in {10, 100, 1000}: thin, scan, similar
  sweep      k = 100, n = 1 .. 8192 in powers of two: thin against scan (the
             source of the FRECSYS_AUDIENCE_THIN_MAX default)
  exclude    k = 100, n in {1, 8, 64} with FRECSYS_AUD_EXCLUDE_HISTORY over the
             synthetic ML-20M CSR (frecsys_hip.data.synthetic)
  big        a 2,000,000 x 256 user table (2 GB: past the 256 MiB Infinity
             Cache), n in {1, 8}, k = 100
  yardstick  the similar() rows of main and big alone: runs on any build
--pkg DIR imports frecsys_hip from DIR (the package of another build); --label
names the build in every line.  One JSON line per case and path: times in ms,
the plan, and table_gbs = passes m Dp 4 bytes / median time.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIN = "FRECSYS_AUDIENCE_THIN_MAX"
REPS, DIM = 5, 256
NS, KS = (1, 8, 64, 1024), (10, 100, 1000)


def _args():
    argv = sys.argv[1:]
    opt = {"--label": "this", "--pkg": os.path.join(ROOT, "safer2-recommender_amd"), "--out": None}
    modes = []
    i = 0
    while i < len(argv):
        if argv[i] in opt:
            opt[argv[i]] = argv[i + 1]
            i += 2
        else:
            modes.append(argv[i])
            i += 1
    return modes or ["main"], opt


MODES, OPT = _args()
sys.path.insert(0, OPT["--pkg"])

import frecsys_hip as fh  # noqa: E402


def _stats(ms):
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms)}


def _timed(ctx, key, call):
    call()  # warm-up: allocations, code load
    ms, launches = [], 0
    for _ in range(REPS):
        ctx.timing_reset()
        call()
        t, launches = ctx.timing(key)
        ms.append(t)
    return ms, launches


def _tables(nu, ni, seed):
    rng = np.random.default_rng(seed)
    s = np.float32(DIM ** -0.25)
    U = rng.standard_normal((nu, DIM), dtype=np.float32) * s
    V = rng.standard_normal((ni, DIM), dtype=np.float32) * s
    return U, V


class Bench:
    def __init__(self, nu, ni, csr=None):
        self.nu, self.ni = nu, ni
        U, V = _tables(nu, ni, 4)
        self.ctx = fh.Context(DIM, nu, ni)
        self.ctx.set_embeddings(fh.SIDE_USER, U)
        self.ctx.set_embeddings(fh.SIDE_ITEM, V)
        if csr is not None:
            self.ctx.load_csr(fh.SIDE_ITEM, *csr)
        self.rng = np.random.default_rng(5)
        self.lines = []

    def emit(self, **line):
        line.update(build=OPT["--label"], users=self.nu, items=self.ni, dim=DIM)
        self.lines.append(json.dumps(line))
        print(self.lines[-1], flush=True)

    def ids(self, n, side_rows):
        return np.sort(self.rng.permutation(side_rows)[:n]).astype(np.int64)

    def audience(self, n, k, path, exclude=False, items=None):
        """path "thin" or "scan": one line, and the lists for a comparison."""
        os.environ[THIN] = "1000000000" if path == "thin" else "0"
        items = self.ids(n, self.ni) if items is None else items
        out = {}
        ms, launches = _timed(self.ctx, "audience", lambda: out.update(
            r=self.ctx.audience(k, items=items, exclude_history=exclude)))
        flops, nbytes = self.ctx.work("audience")[:2]
        pl = fh.audience_plan(DIM, self.nu, n, k, exclude=exclude)
        del os.environ[THIN]
        med = float(np.median(ms)) * 1e-3
        self.emit(call="audience", path=path, n=n, k=k, exclude=exclude, ms=_stats(ms),
                  launch_groups=launches, plan=pl, flops=flops, bytes=nbytes,
                  table_gbs=pl["passes"] * self.nu * DIM * 4.0 / med / 1e9,
                  tflops=flops / med / 1e12)
        return items, out["r"]

    def similar(self, n, k):
        rows = self.ids(n, self.nu)
        ms, launches = _timed(self.ctx, "similar", lambda: self.ctx.similar(
            fh.SIDE_USER, k, rows=rows, cosine=False, keep_self=True))
        med = float(np.median(ms)) * 1e-3
        self.emit(call="similar", path="scan", n=n, k=k, exclude=False, ms=_stats(ms),
                  launch_groups=launches, splits=self.ctx.counter("recommend_splits"),
                  table_gbs=-(-n // 64) * self.nu * DIM * 4.0 / med / 1e9)

    def both(self, n, k, exclude=False, items=None):
        items, thin = self.audience(n, k, "thin", exclude, items)
        _, scan = self.audience(n, k, "scan", exclude, items)
        same = bool((thin[0] == scan[0]).all() and
                    (thin[1].view(np.uint32) == scan[1].view(np.uint32)).all())
        self.emit(call="audience", path="thin==scan", n=n, k=k, exclude=exclude, identical=same)


def main():
    from frecsys_hip.data import SHAPES, synthetic
    shape = SHAPES["ml20m"]
    lines = []
    head = [m for m in MODES if m in ("main", "sweep", "exclude", "yardstick")]
    if head:
        csr = None
        if "exclude" in head:
            _, _, ip, ic = synthetic(shape)
            csr = (ip, ic)
        b = Bench(shape.n_users, shape.n_items, csr)
        for n in NS if ("main" in head or "yardstick" in head) else ():
            for k in KS:
                if "main" in head:
                    b.both(n, k)
                b.similar(n, k)
        if "sweep" in head:
            for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192):
                b.both(n, 100)
        if "exclude" in head:
            ip = csr[0]
            hot = np.argsort(-(ip[1:] - ip[:-1]), kind="stable")    # the longest rows first
            for n in (1, 8, 64):
                items = np.sort(np.concatenate([hot[:max(1, n // 8)],
                                                hot[len(hot) // 2:][:n - max(1, n // 8)]]))
                b.both(n, 100, exclude=True, items=items[:n].astype(np.int64))
        lines += b.lines
        b.ctx.close()
    if "big" in MODES or "yardstick" in MODES:
        b = Bench(2_000_000, shape.n_items)
        for n in (1, 8):
            if "big" in MODES:
                b.both(n, 100)
            b.similar(n, 100)
        lines += b.lines
        b.ctx.close()
    if OPT["--out"]:
        with open(OPT["--out"], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
