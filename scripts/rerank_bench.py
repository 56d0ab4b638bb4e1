#!/usr/bin/env python3
"""Kernel time of frecsys_rank_candidates / frecsys_score_pairs against what a
caller with PyTorch-ROCm writes today on the same device arrays: `V[cand]`
gather, `bmm` (row-wise dot for pairs), `torch.topk`.  The library side is the
HIP-event time of its own timers ("rank_candidates", "score_pairs"), the
yardstick torch events around the composition (in row batches whose gathered
block stays under 16 GiB); one warm-up, then the median / min / max of 5.

  a  116,677 rows x 500 random distinct candidates of 20,108 items, d = 256,
     k = 100
  b  the first 64 rows of the same
  c  1,024 rows x 5,000 random distinct candidates of 500,000 items, d = 1024,
     k = 100
  d  10^7 random pairs at d = 256 (case a's tables) for score_pairs

Usage: rerank_bench.py [a|b|c|d ...] [--out FILE.jsonl]
Prints (and appends to FILE) one JSON line per case: times in ms, the row
batches, frecsys_work's bytes / time as a fraction of the 8 TB/s HBM rate, and
the verdict of the bar: the library's median not above the yardstick's, and
its max not above the yardstick's min by more than the yardstick's spread
(max - min).  No history exclusion and no mask on either side.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

import frecsys_hip as fh  # noqa: E402

K, REPS = 100, 5
HBM_BYTES_PER_S = 8e12
GATHER_CAP = 16 << 30


def _tables(rows, items, dim, seed):
    rng = np.random.default_rng(seed)
    s = dim ** -0.25
    X = rng.standard_normal((rows, dim), dtype=np.float32) * np.float32(s)
    V = rng.standard_normal((items, dim), dtype=np.float32) * np.float32(s)
    return X, V


def _distinct_lists(rows, length, items, seed):
    """[rows, length] int32, every row distinct ids: consecutive runs of
    random permutations of the catalogue."""
    rng = np.random.default_rng(seed)
    per = items // length
    perms = [rng.permutation(items)[:per * length].reshape(per, length)
             for _ in range((rows + per - 1) // per)]
    return np.ascontiguousarray(np.concatenate(perms)[:rows], dtype=np.int32)


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def _timed_lib(ctx, key, call):
    call()  # warm-up: allocations, code load
    ms, launches = [], 0
    for _ in range(REPS):
        ctx.timing_reset()
        call()
        t, launches = ctx.timing(key)
        ms.append(t)
    return ms, launches


def _timed_torch(call):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _verdict(res, lib, ref):
    spread = ref["max"] - ref["min"]
    res["yardstick_spread_ms"] = spread
    res["median_not_slower"] = bool(lib["median"] <= ref["median"])
    res["max_within_spread_of_min"] = bool(lib["max"] - ref["min"] <= spread)
    res["bar_met"] = res["median_not_slower"] and res["max_within_spread_of_min"]
    res["speedup_median"] = ref["median"] / lib["median"]


def run_rank(name, X, V, cand):
    rows, dim = X.shape
    items, length = V.shape[0], cand.shape[1]
    ctx = fh.Context(dim, 1, items)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, np.arange(rows + 1, dtype=np.int64), np.zeros(rows, np.int32))
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    cp = (length * np.arange(rows + 1)).astype(np.int64)
    ci = cand.reshape(-1)
    out = {}
    lib, batches = _timed_lib(ctx, "rank_candidates", lambda: out.update(
        r=ctx.rank_candidates(fh.SIDE_EVAL, K, cp, ci, exclude_history=False)))
    flops, nbytes = ctx.work("rank_candidates")[:2]
    ctx.close()
    Xt, Vt = torch.from_numpy(X).cuda(), torch.from_numpy(V).cuda()
    Ct = torch.from_numpy(cand).cuda().long()
    nb = max(1, min(rows, GATHER_CAP // (length * dim * 4)))

    def compose():
        ids, sc = [], []
        for r0 in range(0, rows, nb):
            c = Ct[r0:r0 + nb]
            s = torch.bmm(Vt[c], Xt[r0:r0 + nb, :, None]).squeeze(-1)
            v, i = torch.topk(s, K, dim=1)
            ids.append(torch.gather(c, 1, i))
            sc.append(v)
        out["t"] = (torch.cat(ids), torch.cat(sc))

    ref = _timed_torch(compose)
    same = float(np.mean(np.all(out["r"][0] == out["t"][0].cpu().numpy(), axis=1)))
    del Xt, Vt, Ct
    out.clear()
    torch.cuda.empty_cache()
    res = {"case": name, "rows": rows, "list": length, "items": items, "dim": dim, "k": K,
           "rank_candidates_ms": _stats(lib), "torch_ms": _stats(ref), "row_batches": batches,
           "torch_row_batches": (rows + nb - 1) // nb,
           "hbm_fraction": nbytes / (float(np.median(lib)) * 1e-3) / HBM_BYTES_PER_S,
           "gflops": flops / (float(np.median(lib)) * 1e-3) / 1e9,
           "rows_identical_to_torch": same}
    _verdict(res, res["rank_candidates_ms"], res["torch_ms"])
    return res


def run_pairs(name, X, V, n_pairs):
    rows, dim = X.shape
    items = V.shape[0]
    rng = np.random.default_rng(5)
    pr = rng.integers(0, rows, n_pairs).astype(np.int64)
    pi = rng.integers(0, items, n_pairs).astype(np.int32)
    ctx = fh.Context(dim, 1, items)
    ctx.set_embeddings(fh.SIDE_ITEM, V)
    ctx.load_csr(fh.SIDE_EVAL, np.arange(rows + 1, dtype=np.int64), np.zeros(rows, np.int32))
    ctx.set_embeddings(fh.SIDE_EVAL, X)
    out = {}
    lib, batches = _timed_lib(ctx, "score_pairs",
                              lambda: out.update(r=ctx.score_pairs(fh.SIDE_EVAL, pr, pi)))
    flops, nbytes = ctx.work("score_pairs")[:2]
    ctx.close()
    Xt, Vt = torch.from_numpy(X).cuda(), torch.from_numpy(V).cuda()
    Rt, It = torch.from_numpy(pr).cuda(), torch.from_numpy(pi).cuda().long()
    ref = _timed_torch(lambda: out.update(t=(Xt[Rt] * Vt[It]).sum(-1)))
    err = float(np.abs(out["r"] - out["t"].cpu().numpy()).max())
    del Xt, Vt, Rt, It
    out.clear()
    torch.cuda.empty_cache()
    res = {"case": name, "pairs": n_pairs, "rows": rows, "items": items, "dim": dim,
           "score_pairs_ms": _stats(lib), "torch_ms": _stats(ref), "pair_batches": batches,
           "hbm_fraction": nbytes / (float(np.median(lib)) * 1e-3) / HBM_BYTES_PER_S,
           "gflops": flops / (float(np.median(lib)) * 1e-3) / 1e9,
           "max_abs_diff_to_torch": err}
    _verdict(res, res["score_pairs_ms"], res["torch_ms"])
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    cases = args or ["a", "b", "c", "d"]

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")

    if set(cases) & {"a", "b", "d"}:
        rows, items, dim = 116_677, 20_108, 256
        X, V = _tables(rows, items, dim, 1)
        if "b" in cases:
            emit(run_rank("b", X[:64], V, _distinct_lists(64, 500, items, 11)))
        if "d" in cases:
            emit(run_pairs("d", X, V, 10_000_000))
        if "a" in cases:
            emit(run_rank("a", X, V, _distinct_lists(rows, 500, items, 12)))
    if "c" in cases:
        rows, items, dim = 1024, 500_000, 1024
        X, V = _tables(rows, items, dim, 2)
        emit(run_rank("c", X, V, _distinct_lists(rows, 5000, items, 13)))


if __name__ == "__main__":
    main()
