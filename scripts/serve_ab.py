"""A/B of the ranking and evaluation calls of libfrecsys_hip.so between two
builds of the library (a refactor's tree and its parent).

    python scripts/serve_ab.py --lib PATH --out A.jsonl [--host-only]
    python scripts/serve_ab.py --join PARENT.jsonl THIS.jsonl --out ab_outputs.jsonl

The first form loads the library at PATH (any build: only the C-ABI is used)
and runs a fixed case table on seeded synthetic data, one JSON line per case:
a SHA-256 of all output bytes, the return code and the last-error text and,
for context calls, work() and the launch count of every timer touched and the
recommend_splits counter.

The second form joins two such files by case name into one short line per case
with an `equal` field (the message, the launch counts and the splits kept, the
rest hashed; both full lines where they differ) and exits non-zero unless every
case is equal.

--host-only runs the context-free functions and, where a device is present,
the defect rows that fail before any device call.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safer2-recommender_amd"))

TIMERS = ("recommend", "rank_metrics", "similar", "similar.norms", "diversify.gram",
          "diversify.select", "dpp.select", "quality", "quality.exposure", "score_pairs",
          "rank_candidates", "sample_negatives", "rank_positions", "explain")
WORK = ("recommend", "rank_metrics", "similar", "diversify", "dpp", "quality", "score_pairs",
        "rank_candidates", "sample_negatives", "rank_positions", "explain")
NU, NI, K, POOL = 165, 3000, 10, 96   # rows = users; POOL: 36 KiB of Gramian a row
KS = (3, 10)
ENV = ("FRECSYS_RECOMMEND_WS_MB", "FRECSYS_RECOMMEND_SPLITS", "FRECSYS_DIVERSIFY_VARIANT",
       "FRECSYS_DPP_FACTOR")


def digest(outs):
    h = hashlib.sha256()
    for a in outs:
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class Runner:
    def __init__(self, fh, out):
        self.fh, self.lib, self.out, self.ctx = fh, fh.load_library(), out, None

    def emit(self, name, rc, err, outs, extra=None):
        line = {"case": name, "rc": rc, "error": err, "sha256": digest(outs)}
        line.update(extra or {})
        self.out.write(json.dumps(line) + "\n")
        return line

    def host(self, name, fn, outs, *args):
        """A context-free call: fn(*args) -> rc; outs are its output arrays."""
        rc = getattr(self.lib, fn)(*[self.fh._ptr(a) if isinstance(a, np.ndarray) else a
                                     for a in args])
        self.emit(name, rc, self.lib.frecsys_last_error(None).decode() if rc else "", outs)

    def raw(self, name, fn, outs, *args):
        """A context call through the C-ABI as it is (defect rows)."""
        c = self.ctx
        rc = getattr(self.lib, fn)(c.h, *[self.fh._ptr(a) if isinstance(a, np.ndarray) else a
                                          for a in args])
        self.emit(name, rc, self.lib.frecsys_last_error(c.h).decode() if rc else "", outs)

    def call(self, name, fn, env=None):
        """A context call through the Context method: fn() -> output arrays."""
        c = self.ctx
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(env or {})
        c.timing_reset()
        try:
            outs, rc, err = fn(), 0, ""
            outs = list(outs.values()) if isinstance(outs, dict) else list(outs)
        except self.fh.FrecsysError as e:
            outs, rc, err = [], e.code, str(e)
        return self.emit(name, rc, err, outs, {
            "work": {k: c.work(k) for k in WORK if c.work(k)[3]},
            "launches": {k: c.timing(k)[1] for k in TIMERS if c.timing(k)[1]},
            "recommend_splits": c.counter("recommend_splits")})


def synthetic(d, seed):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((NU, d)).astype(np.float32) * 0.3
    V = rng.standard_normal((NI, d)).astype(np.float32) * 0.3
    V[7] = 0.0                                                    # a zero-norm item
    hist = [np.sort(rng.choice(NI, size=int(rng.integers(1, 40)), replace=False)) for _ in range(NU)]
    up = np.concatenate([[0], np.cumsum([len(h) for h in hist])]).astype(np.int64)
    uc = np.concatenate(hist).astype(np.int32)
    order = np.argsort(uc, kind="stable")
    ip = np.concatenate([[0], np.cumsum(np.bincount(uc, minlength=NI))]).astype(np.int64)
    ic = np.repeat(np.arange(NU), np.diff(up))[order].astype(np.int32)
    gt = [rng.choice(NI, size=int(rng.integers(1, 6))) for _ in range(NU)]   # repeats allowed
    gp = np.concatenate([[0], np.cumsum([len(g) for g in gt])]).astype(np.int64)
    gi = np.concatenate(gt).astype(np.int32)
    cand = [rng.choice(NI, size=int(rng.integers(0, 60))) for _ in range(NU)]
    cp = np.concatenate([[0], np.cumsum([len(g) for g in cand])]).astype(np.int64)
    ci = np.concatenate(cand).astype(np.int32)
    mask = (rng.random(NI) < 0.7).astype(np.uint8)
    rows = rng.integers(0, NU, size=NU).astype(np.int64)          # any order, repeats
    weight = rng.random(NI).astype(np.float32)
    pools = rng.integers(-1, NI, size=(NU, POOL)).astype(np.int32)
    pools[3, :] = -1                                              # an empty pool
    pools[4, K:] = -1                                             # exactly k filled slots
    pscores = rng.standard_normal((NU, POOL)).astype(np.float32)
    lists = rng.integers(-1, NI, size=(NU, 12)).astype(np.int32)
    return dict(U=U, V=V, up=up, uc=uc, ip=ip, ic=ic, gp=gp, gi=gi, cp=cp, ci=ci, mask=mask,
                rows=rows, weight=weight, pools=pools, pscores=pscores, lists=lists)


def host_cases(r, d, D):
    fh, P = r.fh, f"host d{d} "
    V, pools, ps, lists = D["V"], D["pools"], D["pscores"], D["lists"]
    n = NU
    for raw in (0, fh.DIV_RAW_SCORES):
        for k in (K, POOL):
            it, sc, x = (np.zeros((n, k), np.int32), np.zeros((n, k), np.float32),
                         np.zeros((n, k), np.float32))
            r.host(f"{P}mmr_select raw{raw} k{k}", "frecsys_mmr_select", [it, sc, x], V, NI, d, d,
                   pools, ps, n, POOL, k, 0.6, raw, it, sc, x)
            r.host(f"{P}mmr_select raw{raw} k{k} no mmr", "frecsys_mmr_select", [it, sc], V, NI, d,
                   d, pools, ps, n, POOL, k, 0.6, raw, it, sc, None)
            for eps in (1e-3, 0.5):
                r.host(f"{P}dpp_select raw{raw} k{k} eps{eps}", "frecsys_dpp_select", [it, sc, x],
                       V, NI, d, d, pools, ps, n, POOL, k, 3.0, eps, raw, it, sc, x)
    ks = np.array(KS, np.int32)
    ild, nov = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    ex = np.zeros((2, NI), np.int64)
    r.host(P + "list_quality", "frecsys_list_quality", [ild, nov, ex], V, NI, d, d, lists, n, 12,
           ks, 2, D["weight"], ild, nov, ex)
    r.host(P + "list_quality exposure only", "frecsys_list_quality", [ex], None, NI, d, d, lists,
           n, 12, ks, 2, None, None, None, ex)
    cov, gini = ctypes.c_double(), ctypes.c_double()
    tot, cvd = ctypes.c_int64(), ctypes.c_int64()
    rc = r.lib.frecsys_exposure_summary(fh._ptr(ex[1]), NI, fh._ptr(D["mask"]), ctypes.byref(cov),
                                        ctypes.byref(gini), ctypes.byref(tot), ctypes.byref(cvd))
    r.emit(P + "exposure_summary", rc, "",
           [np.array([cov.value, gini.value]), np.array([tot.value, cvd.value])])
    rec, nd = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    r.host(P + "list_metrics", "frecsys_list_metrics", [rec, nd], lists, n, 12, D["gp"], D["gi"],
           ks, 2, rec, nd)
    cnt, neg = np.zeros(n, np.int32), np.zeros((n, 20), np.int32)
    for tag, mk, rows in (("", None, None), (" mask rows", D["mask"], D["rows"])):
        r.host(P + "sample_negatives" + tag, "frecsys_sample_negatives", [cnt, neg], NI, mk, rows,
               n, D["up"], D["uc"], D["gp"], D["gi"], 20, 12345, cnt, neg)
    rank = np.minimum(np.arange(len(D["gi"]), dtype=np.int32) % 50 - 1, 40)
    elig = np.full(n, 41, np.int32)
    mrr, auc = np.zeros(n, np.float32), np.zeros(n, np.float32)
    r.host(P + "position_metrics", "frecsys_position_metrics", [mrr, auc], rank, D["gp"], elig, n,
           mrr, auc)
    vals, al, out = nd[:, 1].copy(), np.array([0.1, 0.5, 0.9], np.float32), np.zeros(3, np.float32)
    r.host(P + "metric_cvar", "frecsys_metric_cvar", [out], vals, n, al, 3, out)
    if d != 8:
        return
    # defect rows, one defect each (they do not depend on d)
    it, sc = np.zeros((n, K), np.int32), np.zeros((n, K), np.float32)
    bad_id, bad_sc = pools.copy(), ps.copy()
    bad_id[2, 1], bad_sc[2, np.argmax(pools[2] >= 0)] = NI, np.inf
    sel = lambda **o: dict(dict(V=V, ni=NI, dim=d, ld=d, ls=pools, sc=ps, n=n, pool=POOL, k=K,
                                flags=0, it=it, out=sc), **o)
    defects = [("k 0", sel(k=0)), ("k above pool", sel(k=POOL + 1)), ("pool 0", sel(pool=0)),
               ("pool 2000", sel(pool=2000)), ("unknown flag", sel(flags=8)),
               ("negative n", sel(n=-1)), ("zero rows", sel(n=0)), ("null table", sel(V=None)),
               ("ld below dim", sel(ld=d - 1)), ("null lists", sel(ls=None)),
               ("null items", sel(it=None)), ("id out of range", sel(ls=bad_id)),
               ("non-finite score", sel(sc=bad_sc))]
    for tag, a in defects:
        head = (a["V"], a["ni"], a["dim"], a["ld"], a["ls"], a["sc"], a["n"], a["pool"], a["k"])
        r.host(f"{P}mmr_select defect {tag}", "frecsys_mmr_select", [], *head, 0.5, a["flags"],
               a["it"], a["out"], None)
        r.host(f"{P}dpp_select defect {tag}", "frecsys_dpp_select", [], *head, 1.0, 1e-3,
               a["flags"], a["it"], a["out"], None)
    for tag, lam in (("lam nan", np.nan), ("lam 1.5", 1.5)):
        r.host(f"{P}mmr_select defect {tag}", "frecsys_mmr_select", [], V, NI, d, d, pools, ps, n,
               POOL, K, lam, 0, it, sc, None)
    for tag, th, eps in (("theta inf", np.inf, 1e-3), ("theta negative", -1.0, 1e-3),
                         ("eps 0", 1.0, 0.0), ("eps nan", 1.0, np.nan)):
        r.host(f"{P}dpp_select defect {tag}", "frecsys_dpp_select", [], V, NI, d, d, pools, ps, n,
               POOL, K, th, eps, 0, it, sc, None)
    bad_w, bad_l = D["weight"].copy(), lists.copy()
    bad_w[5], bad_l[1, 1] = np.nan, NI
    lq = lambda **o: dict(dict(V=V, ni=NI, ls=lists, n=n, lk=12, ks=ks, nk=2, w=D["weight"],
                               ild=ild, nov=nov, ex=ex), **o)
    for tag, a in [("list_k 0", lq(lk=0)), ("no items", lq(ni=0)), ("null k_list", lq(ks=None)),
                   ("nk 33", lq(nk=33)), ("cut-off above list_k", lq(lk=5)),
                   ("every output null", lq(ild=None, nov=None, ex=None, w=None)),
                   ("novelty without weight", lq(w=None)), ("weight without novelty", lq(nov=None)),
                   ("non-finite weight", lq(w=bad_w)), ("null table", lq(V=None)),
                   ("negative n", lq(n=-1)), ("null lists", lq(ls=None)),
                   ("id out of range", lq(ls=bad_l)), ("zero rows", lq(n=0))]:
        r.host(f"{P}list_quality defect {tag}", "frecsys_list_quality",
               [a["ex"]] if tag == "zero rows" else [], a["V"], a["ni"], d, d, a["ls"], a["n"],
               a["lk"], a["ks"], a["nk"], a["w"], a["ild"], a["nov"], a["ex"])
    bad_gp = D["gp"].copy()
    bad_gp[3] = bad_gp[2]
    r.host(P + "list_metrics defect empty row", "frecsys_list_metrics", [], lists, n, 12, bad_gp,
           D["gi"], ks, 2, rec, nd)
    r.host(P + "list_metrics defect list_k below cut-off", "frecsys_list_metrics", [], lists, n, 5,
           D["gp"], D["gi"], ks, 2, rec, nd)
    r.host(P + "position_metrics defect rank", "frecsys_position_metrics", [], rank + 100, D["gp"],
           elig, n, mrr, auc)
    r.host(P + "sample_negatives defect n_neg", "frecsys_sample_negatives", [], NI, None, None, n,
           None, None, D["gp"], D["gi"], -1, 0, cnt, neg)
    r.host(P + "metric_cvar defect", "frecsys_metric_cvar", [], None, 3, al, 3, out)
    r.host(P + "exposure_summary defect", "frecsys_exposure_summary", [], None, NI, None, None,
           None, None, None)


def defect_cases(r, d, D):
    """Context calls that fail before any device call: one defect each."""
    P, n = f"defect d{d} ", NU
    it, sc = np.zeros((n, K), np.int32), np.zeros((n, K), np.float32)
    ks = np.array(KS, np.int32)
    ild, nov = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    rec, nd = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    ex = np.ones((2, NI), np.int64)
    pools, ps = D["pools"], D["pscores"]
    bad_id, bad_sc, bad_rows = pools.copy(), ps.copy(), D["rows"].copy()
    bad_id[2, 1], bad_sc[2, np.argmax(pools[2] >= 0)], bad_rows[9] = NI, np.nan, NU
    rd = lambda **o: dict(dict(side=0, rows=None, n=n, k=K, pool=POOL, x=0.5, eps=1e-3, flags=0,
                               mask=None, it=it, sc=sc), **o)
    for tag, a in [("k 0", rd(k=0)), ("k above pool", rd(k=POOL + 1)), ("pool 0", rd(pool=0)),
                   ("pool 1025", rd(pool=1025)), ("unknown flag", rd(flags=4)),
                   ("bad side", rd(side=1)), ("negative n", rd(n=-1)), ("null items", rd(it=None)),
                   ("null scores", rd(sc=None)), ("row id out of range", rd(rows=bad_rows)),
                   ("more rows than the side", rd(n=n + 1)), ("zero rows", rd(n=0)),
                   ("exclude without csr", rd(side=2, flags=1))]:
        head = (a["side"], a["rows"], a["n"], a["k"], a["pool"])
        tail = (a["flags"], a["mask"], a["it"], a["sc"], None)
        r.raw(f"{P}recommend_diverse {tag}", "frecsys_recommend_diverse", [], *head, a["x"], *tail)
        r.raw(f"{P}recommend_dpp {tag}", "frecsys_recommend_dpp", [], *head, a["x"], a["eps"],
              *tail)
    for tag, lam in (("lam nan", np.nan), ("lam -0.1", -0.1)):
        r.raw(f"{P}recommend_diverse {tag}", "frecsys_recommend_diverse", [], 0, None, n, K, POOL,
              lam, 0, None, it, sc, None)
        r.raw(f"{P}diversify {tag}", "frecsys_diversify", [], pools, ps, n, POOL, K, lam, 0, it, sc,
              None)
    for tag, th, eps in (("theta nan", np.nan, 1e-3), ("theta negative", -1.0, 1e-3),
                         ("eps 0", 1.0, 0.0), ("eps 1.5", 1.0, 1.5)):
        r.raw(f"{P}recommend_dpp {tag}", "frecsys_recommend_dpp", [], 0, None, n, K, POOL, th, eps,
              0, None, it, sc, None)
        r.raw(f"{P}diversify_dpp {tag}", "frecsys_diversify_dpp", [], pools, ps, n, POOL, K, th,
              eps, 0, it, sc, None)
    dv = lambda **o: dict(dict(ls=pools, ps=ps, n=n, pool=POOL, k=K, flags=0, it=it, sc=sc), **o)
    for tag, a in [("k 0", dv(k=0)), ("k above pool", dv(k=POOL + 1)), ("pool 0", dv(pool=0)),
                   ("unknown flag", dv(flags=1)), ("negative n", dv(n=-1)), ("zero rows", dv(n=0)),
                   ("null lists", dv(ls=None)), ("null scores in", dv(ps=None)),
                   ("null items", dv(it=None)), ("null scores out", dv(sc=None)),
                   ("id out of range", dv(ls=bad_id)), ("non-finite score", dv(ps=bad_sc))]:
        head = (a["ls"], a["ps"], a["n"], a["pool"], a["k"])
        r.raw(f"{P}diversify {tag}", "frecsys_diversify", [], *head, 0.5, a["flags"], a["it"],
              a["sc"], None)
        r.raw(f"{P}diversify_dpp {tag}", "frecsys_diversify_dpp", [], *head, 1.0, 1e-3, a["flags"],
              a["it"], a["sc"], None)
    bad_w, bad_gi, bad_l = D["weight"].copy(), D["gi"].copy(), D["lists"].copy()
    bad_w[11], bad_gi[4], bad_l[2, 2] = np.inf, NI, NI + 5
    rq = lambda **o: dict(dict(side=0, rows=None, n=n, flags=0, mask=None, ks=ks, nk=2, pool=0,
                               lam=0.5, dfl=0, w=D["weight"], gp=D["gp"], gi=D["gi"], ild=ild,
                               nov=nov, rec=rec, nd=nd, ex=ex), **o)
    no_out = dict(ild=None, nov=None, w=None, ex=None, gp=None, gi=None, rec=None, nd=None)
    for tag, a in [("null k_list", rq(ks=None)), ("nk 0", rq(nk=0)),
                   ("cut-off 2000", rq(ks=np.array([3, 2000], np.int32))),
                   ("every output null", rq(**no_out)), ("novelty without weight", rq(w=None)),
                   ("weight without novelty", rq(nov=None)), ("non-finite weight", rq(w=bad_w)),
                   ("metrics without ground truth", rq(gp=None, gi=None)),
                   ("ground truth without ndcg", rq(nd=None)), ("pool below k", rq(pool=5)),
                   ("pool 1025", rq(pool=1025)), ("lam 2", rq(pool=POOL, lam=2.0)),
                   ("div flag unknown", rq(pool=POOL, dfl=1)), ("div flags without pool", rq(dfl=2)),
                   ("negative n", rq(n=-1)), ("bad side", rq(side=1)), ("unknown flag", rq(flags=2)),
                   ("row id out of range", rq(rows=bad_rows)),
                   ("ground-truth id out of range", rq(gi=bad_gi)),
                   ("zero rows with exposure", rq(n=0, gp=None, gi=None, rec=None, nd=None))]:
        a["ex"] = None if a["ex"] is None else np.ones((2, NI), np.int64)
        r.raw(f"{P}rank_quality {tag}", "frecsys_rank_quality", [a["ex"]], a["side"], a["rows"],
              a["n"], a["flags"], a["mask"], a["ks"], a["nk"], a["pool"], a["lam"], a["dfl"], a["w"],
              a["gp"], a["gi"], a["ild"], a["nov"], a["rec"], a["nd"], a["ex"])
    lq = lambda **o: dict(dict(ls=D["lists"], n=n, lk=12, ks=ks, nk=2, w=D["weight"], ild=ild,
                               nov=nov, ex=ex), **o)
    for tag, a in [("list_k 0", lq(lk=0)), ("null k_list", lq(ks=None)), ("nk 33", lq(nk=33)),
                   ("cut-off above list_k", lq(lk=5)),
                   ("every output null", lq(ild=None, nov=None, ex=None, w=None)),
                   ("novelty without weight", lq(w=None)), ("weight without novelty", lq(nov=None)),
                   ("non-finite weight", lq(w=bad_w)), ("negative n", lq(n=-1)),
                   ("null lists", lq(ls=None)), ("overflow", lq(n=2 ** 62, ls=D["lists"])),
                   ("id out of range", lq(ls=bad_l)), ("zero rows with exposure", lq(n=0))]:
        a["ex"] = None if a["ex"] is None else np.ones((2, NI), np.int64)
        r.raw(f"{P}lists_quality {tag}", "frecsys_lists_quality", [a["ex"]], a["ls"], a["n"],
              a["lk"], a["ks"], a["nk"], a["w"], a["ild"], a["nov"], a["ex"])


def device_cases(r, d, D):
    fh, c = r.fh, r.ctx
    gp, gi, cp, ci = D["gp"], D["gi"], D["cp"], D["ci"]
    for ws in (None, "1"):
        # 1 MiB: the default splits give batches of about ten rows, as many as the
        # Gramians of a sub-batch; the calls with a pool also fix two item splits,
        # so that their scan batch is one 64-row block of several sub-batches
        wenv = {} if ws is None else {"FRECSYS_RECOMMEND_WS_MB": ws}
        penv = dict(wenv, **({"FRECSYS_RECOMMEND_SPLITS": "2"} if ws else {}))
        # the options together and, at d = 8, exclusion alone and row ids alone
        combos = ((0, 0, 0), (1, 1, 1)) + (((1, 0, 0), (0, 0, 1)) if d == 8 else ())
        for ex, mk, rw in combos:
            P = f"d{d} ws{ws or 'default'} excl{ex} mask{mk} rows{rw} "
            q = dict(rows=D["rows"] if rw else None, exclude_history=bool(ex),
                     item_mask=D["mask"] if mk else None)
            hist = 16 * ((NI + 127) // 128) if ex else 0   # history bits of a row

            def scan(name, fn, env, k, extra, gram=False):
                line = r.call(P + name, fn, env)
                if ws:
                    check_batches(line, k, extra + hist)
                    # the Gramian sub-batch is smaller than the batch
                    assert not gram or (line["launches"]["diversify.gram"]
                                        > line["launches"]["recommend"]), line

            scan("recommend", lambda: c.recommend(0, K, **q), wenv, K, 0)
            scan("rank_metrics", lambda: c.rank_metrics(0, KS, gp, gi, **q), wenv, K, 8 * len(KS))
            for cos in (False, True):
                for keep in (False, True):
                    line = r.call(f"{P}similar cos{int(cos)} keep{int(keep)}",
                                  lambda: c.similar(1, K, rows=q["rows"], cosine=cos,
                                                    keep_self=keep, mask=q["item_mask"]), wenv)
                    if ws:  # scan_plan's splits for the rows of the call, on 256 CUs
                        n = NU if rw else NI
                        check_batches(dict(line, recommend_splits=min(
                            (NI + 127) // 128, -(-2 * 256 // -(-n // 64)))), K, 0, n, "similar")
            for var in ("gram", "lazy"):
                for raw in (False, True):
                    for third in (False, True):
                        env = dict(penv, FRECSYS_DIVERSIFY_VARIANT=var)
                        t = f"{var} raw{int(raw)} mmr{int(third)}"
                        scan(f"recommend_diverse {t}", lambda: c.recommend_diverse(
                            0, K, POOL, 0.6, raw_scores=raw, return_mmr=third, **q), env, POOL,
                            12 * K, var == "gram")
                        if (ex, mk, rw) == (0, 0, 0):
                            r.call(f"d{d} ws{ws or 'default'} diversify {t}", lambda: c.diversify(
                                D["pools"], D["pscores"], K, 0.6, raw_scores=raw,
                                return_mmr=third), env)
            for fac in (None, "ws"):
                for third in (False, True):
                    env = dict(penv, **({"FRECSYS_DPP_FACTOR": fac} if fac else {}))
                    t = f"factor-{fac or 'default'} gain{int(third)}"
                    scan(f"recommend_dpp {t}", lambda: c.recommend_dpp(
                        0, K, POOL, 3.0, 1e-3, return_gain=third, **q), env, POOL, 12 * K, True)
                    if (ex, mk, rw) == (0, 0, 0):
                        r.call(f"d{d} ws{ws or 'default'} diversify_dpp {t}",
                               lambda: c.diversify_dpp(D["pools"], D["pscores"], K, 3.0, 1e-3,
                                                       return_gain=third), env)
            for pool in (None, POOL):
                for gt in (None, (gp, gi)):
                    scan(f"rank_quality pool{int(pool is not None)} gt{int(gt is not None)}",
                         lambda: c.rank_quality(0, KS, pool=pool, lam=0.6, item_weight=D["weight"],
                                                gt=gt, **q), penv if pool else wenv, pool or K,
                         8 * len(KS) * (2 if gt else 1) + (12 * K if pool else 0), pool is not None)
            scan("rank_quality exposure only", lambda: c.rank_quality(0, KS, ild=False, **q), wenv,
                 K, 8 * len(KS))
            # the controls
            r.call(P + "rank_candidates", lambda: c.rank_candidates(0, K, cp, ci, **q), wenv)
            r.call(P + "rank_candidates_metrics",
                   lambda: c.rank_candidates_metrics(0, KS, cp, ci, gp, gi, **q), wenv)
            r.call(P + "sampled_metrics", lambda: c.sampled_metrics(
                0, KS, gp, gi, 20, seed=7, return_negatives=True, **q), wenv)
            r.call(P + "rank_positions", lambda: c.rank_positions(0, gp, gi, **q), wenv)
        P = f"d{d} ws{ws or 'default'} "
        r.call(P + "lists_quality", lambda: c.lists_quality(D["lists"], KS, D["weight"]), wenv)
        r.call(P + "score_pairs", lambda: c.score_pairs(0, D["rows"], ci[:NU]), wenv)
        tp = np.concatenate([[0], np.cumsum(np.minimum(np.diff(cp), 3))]).astype(np.int64)
        ti = np.concatenate([ci[cp[i]:cp[i] + min(3, cp[i + 1] - cp[i])] for i in range(NU)])
        r.call(P + "explain", lambda: c.explain(0, fh.KIND_IALS, 0.01, 0.1, tp, ti.astype(np.int32),
                                                top=5, full=True)[:4], wenv)


def check_batches(line, k, extra, n=NU, timer="recommend", budget=1 << 20):
    """The 1 MiB shape: by scan_plan's formula (cap = 4 k to a power of two in
    [512, 2048]; `extra` bytes a row behind the scan's own) the n rows make at
    least three batches with a partial last one, and the call launched them."""
    cap = 512
    while cap < 4 * k and cap < 2048:
        cap <<= 1
    splits = line["recommend_splits"]
    nb = max(1, budget // (splits * cap * 8 + splits * 4 + k * 8 + extra))
    if nb < n and nb >= 64:
        nb &= ~63
    nb = min(nb, n)
    assert -(-n // nb) >= 3 and n % nb != 0, (line["case"], nb)
    assert line["launches"][timer] == -(-n // nb), (line, nb)


def run(args):
    import frecsys_hip as fh
    fh.load_library(args.lib)
    with open(args.out, "w") as out:
        r = Runner(fh, out)
        for d in (8, 64):
            D = synthetic(d, 100 + d)
            host_cases(r, d, D)
            if args.host_only and fh.device_count() < 1:
                continue
            c = r.ctx = fh.Context(d, NU, NI, device=0)
            c.load_csr(fh.SIDE_USER, D["up"], D["uc"])
            c.load_csr(fh.SIDE_ITEM, D["ip"], D["ic"])
            c.set_embeddings(fh.SIDE_USER, D["U"])
            c.set_embeddings(fh.SIDE_ITEM, D["V"])
            if d == 8:  # they do not depend on d
                defect_cases(r, d, D)
            if not args.host_only:
                c.gramian(fh.SIDE_ITEM, fetch=False)
                device_cases(r, d, D)
            c.close()
    return 0


def join(args):
    a, b = ([json.loads(s) for s in open(p)] for p in args.join)
    bb = {x["case"]: x for x in b}
    assert len(bb) == len(b) == len(a), "case names differ or repeat"
    bad = 0
    with open(args.out, "w") as out:
        for x in a:
            y = bb[x["case"]]
            bad += x != y
            if x == y:  # short: hashes of the outputs and of the whole line (work() too)
                rest = hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()
                line = {"case": x["case"], "equal": True, "rc": x["rc"], "error": x["error"],
                        "sha256": x["sha256"][:16], "line": rest[:16]}
                line.update({k: x[k] for k in ("launches", "recommend_splits") if k in x})
            else:
                line = {"case": x["case"], "equal": False, "parent": x, "this": y}
            out.write(json.dumps(line) + "\n")
    print(f"{len(a)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out", required=True)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--join", nargs=2, metavar=("PARENT", "THIS"))
    a = ap.parse_args()
    sys.exit(join(a) if a.join else run(a))
