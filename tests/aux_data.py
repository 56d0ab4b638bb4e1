"""Deterministic inputs for the kernels around the solve: the Gramian, the
per-user loss, the train statistics, the snapshot residual and the fold-in
top-K (tests/test_aux_cpu.py, tests/test_aux_gpu.py, tests/test_topk_gpu.py).

aux_users()          121 users over the 704 items of seam_data: every seam
                     history (h = 1, 2, 32 t - 1 | 32 t | 32 t + 1 up to 513,
                     639, 640, repeats, first / last item), h = 3..18 one by
                     one (the loss gathers' 2 | 4 | 8 | 16 rows in flight), and
                     idle users at index 0, 61 (the middle), 114 and 120.
                     121 = 4 * 30 + 1 (one wave of the last loss workgroup),
                     past one 64-row quad tile and no multiple of 64.
scaled_embeddings()  fp32 N(0, s^2) tables with s^4 dim = 0.25: predictions
                     x.u have standard deviation 0.5, so (x.u - 1)^2 moves in
                     its first digit when one gathered row is the wrong one
                     (the 0.1 init gives predictions of 6e-4).
aux_eval()           the EVAL CSR of a top-K case.
gram_rows()          the rows / weights of a Gramian case.
"""
import numpy as np

import numpy_ref as R
import seam_data as S

N_USERS = 121
IDLE = (0, 61, 114, 120)
SMALL_H = tuple(range(3, 19))
EVAL_ROWS = 70  # the loss's EVAL case: users 1..70 (EVAL row 0 is not empty)

_cache = {}


def aux_users():
    """(n_users, n_items, up, uc, ip, ic)."""
    if "users" not in _cache:
        from frecsys_hip.data import _csr_from_pairs
        sd = S.make_seam_data()
        rng = np.random.default_rng(41)
        hists = list(sd.hists[:-1])  # the trailing idle entity goes back on at the end
        for h in SMALL_H:
            if h == 14:
                hists.append(np.zeros(0, np.int64))
            hists.append(rng.permutation(sd.n_other)[:h])
        hists.append(np.zeros(0, np.int64))
        ent = np.concatenate([np.full(len(h), e, np.int64) for e, h in enumerate(hists)])
        oth = np.concatenate(hists)
        up, uc = _csr_from_pairs(ent, oth, len(hists))
        ip, ic = _csr_from_pairs(oth, ent, sd.n_other)
        for a in (up, uc, ip, ic):
            a.setflags(write=False)
        _cache["users"] = (len(hists), sd.n_other, up, uc, ip, ic)
    return _cache["users"]


def scaled_embeddings(dim, nu, ni, seed):
    """(U, V) fp32, N(0, s^2) with s^4 dim = 0.25."""
    s = (0.25 / dim) ** 0.25
    rng = np.random.default_rng(seed)
    U = (s * rng.standard_normal((nu, dim))).astype(np.float32)
    V = (s * rng.standard_normal((ni, dim))).astype(np.float32)
    return U, V


def eval_slice(up, uc, lo=1, n=EVAL_ROWS):
    """The CSR of users lo .. lo + n - 1 as an EVAL side."""
    ep = (up[lo:lo + n + 1] - up[lo]).astype(np.int64)
    ec = np.asarray(uc[up[lo]:up[lo + n]], np.int32)
    return ep, ec


def aux_eval(n_rows, n_items, k, seed):
    """(ep, ec): row 0 empty; row 1 {0, n_items - 1}; row 2 with repeated ids;
    row 3 n_items - k + 1 distinct ids (k - 1 items stay free: one excluded
    item has to be listed); the others 1..40 random distinct ids."""
    rng = np.random.default_rng(seed)
    hists = []
    for r in range(n_rows):
        if r == 0:
            h = []
        elif r == 1:
            h = [0, n_items - 1]
        elif r == 2:
            a = rng.integers(0, n_items, 6)
            h = np.concatenate([a, a[:3], a[1:2]])
        elif r == 3 and n_items - k + 1 >= 1:
            h = rng.permutation(n_items)[:n_items - k + 1]
        else:
            h = rng.permutation(n_items)[:min(n_items, int(rng.integers(1, 41)))]
        hists.append(np.asarray(h, np.int32))
    ep = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    ec = np.concatenate(hists).astype(np.int32) if ep[-1] else np.zeros(0, np.int32)
    return ep, ec


# ---- top-K cases ----
TOPK_M = (1, 127, 128, 129, 255, 256, 257, 1024, 1025)
TOPK_ROWS = (1, 63, 64, 65)
TOPK_DIMS = (5, 20, 64, 200, 500)
TOPK_KINDS = ("one", "k33", "max")  # k = 1, 33, min(m, 1024)
TIE_CASES = ("test_topk_ties_straddle_kth",)  # exempt from the gap condition: ties on purpose


def topk_k(m, kind):
    return {"one": 1, "k33": 33 if m >= 33 else 1, "max": min(m, 1024)}[kind]


def topk_plan():
    """(m, rows, kind, dim, seed): every item count at every dim, the row
    counts and the k kinds rotated so that every pair of values of two
    parameters occurs (test_aux_cpu checks the cover)."""
    out = []
    for i, m in enumerate(TOPK_M):
        for j, dim in enumerate(TOPK_DIMS):
            rows = TOPK_ROWS[(i + j) % 4]
            kind = TOPK_KINDS[(i + 2 * j) % 3]
            out.append((m, rows, kind, dim, 1000 + 10 * i + j))
    return out


def topk_cases():
    """(m, rows, k, dim, seed) of topk_plan()."""
    return [(m, rows, topk_k(m, kind), dim, seed) for m, rows, kind, dim, seed in topk_plan()]


def topk_inputs(m, rows, k, dim, seed):
    """(Ue, V, ep, ec, S, ref, close): N(0, 1 / sqrt(dim)) tables (scores of
    standard deviation 1), the EVAL CSR, the float64 scores and ranking, and
    the rows the gap condition flags.  A row whose float64 ranking has two
    listed scores within 2e-6 max|S| is drawn again (its own stream, up to 400
    times): at k = 1024 a Gaussian row has two such scores more often than
    not, and a flagged row is only checked loosely."""
    key = ("topk", m, rows, k, dim, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        s = dim ** -0.25
        V = (s * rng.standard_normal((m, dim))).astype(np.float32)
        Ue = (s * rng.standard_normal((rows, dim))).astype(np.float32)
        ep, ec = aux_eval(rows, m, k, seed + 1)
        for _ in range(400):
            Sc, ref = R.topk64(Ue, V, ep, ec, k)
            close, _ = R.topk_close_rows(Sc, k)
            if not close.any():
                break
            Ue[close] = (s * rng.standard_normal((int(close.sum()), dim))).astype(np.float32)
        for a in (Ue, V, ep, ec, Sc, ref, close):
            a.setflags(write=False)
        _cache[key] = (Ue, V, ep, ec, Sc, ref, close)
    return _cache[key]


# ---- Gramian cases ----
GRAM_DIMS = (5, 16, 20, 50, 64, 96, 128, 160, 192, 224, 256)
GRAM_ROWS = (1, 31, 32, 33, 63, 64, 65, 97, 1024, 1025, 1089)
GRAM_BIG = 32769  # the first row count with 96-row leaves (342 of them)
GRAM_BIG_DIMS = (8, 32, 256)
GRAM_WIDE_DIMS = (500, 1000)
GRAM_WIDE_ROWS = (1, 15, 16, 17, 255, 256, 257, 4097)
GRAM_TOL = 2e-6
# (dim, rows): the fp32 C oracle's own error against float64 on the scale of
# gram_err (the larger of unweighted / weighted, rounded up), listed where it
# is past a quarter of GRAM_TOL: the oracle sums 4,096 rows in sequence, which
# at 1,024 rows and more is 1e-6 by itself.  The bar of such a case is 4 x
# this number instead (2.1e-6 .. 1.3e-5); test_aux_cpu.test_oracle_gramian_share
# holds the oracle to it and to a quarter of GRAM_TOL everywhere else.
GRAM_ORACLE_ERR = {
    (5, 1024): 8.72e-07, (5, 1025): 9.92e-07, (5, 1089): 5.22e-07, (16, 1024): 1.20e-06,
    (16, 1025): 1.34e-06, (16, 1089): 9.41e-07, (20, 1024): 1.35e-06, (20, 1025): 1.13e-06,
    (20, 1089): 1.11e-06, (50, 1024): 1.13e-06, (50, 1025): 1.25e-06, (50, 1089): 1.23e-06,
    (64, 1024): 1.13e-06, (64, 1025): 1.11e-06, (64, 1089): 1.26e-06, (96, 97): 5.63e-07,
    (96, 1024): 1.31e-06, (96, 1025): 1.27e-06, (96, 1089): 1.54e-06, (128, 65): 5.02e-07,
    (128, 1024): 1.63e-06, (128, 1025): 1.20e-06, (128, 1089): 1.38e-06, (160, 1024): 1.27e-06,
    (160, 1025): 1.33e-06, (160, 1089): 1.14e-06, (192, 1024): 1.12e-06, (192, 1025): 1.23e-06,
    (192, 1089): 1.63e-06, (224, 97): 5.03e-07, (224, 1024): 1.44e-06, (224, 1025): 1.30e-06,
    (224, 1089): 1.65e-06, (256, 1024): 1.49e-06, (256, 1025): 1.48e-06, (256, 1089): 1.57e-06,
    (8, 32769): 7.64e-07, (32, 32769): 8.70e-07, (256, 32769): 1.09e-06, (500, 255): 7.33e-07,
    (500, 256): 6.87e-07, (500, 257): 8.29e-07, (500, 4097): 2.99e-06, (1000, 255): 7.86e-07,
    (1000, 256): 8.44e-07, (1000, 257): 7.61e-07, (1000, 4097): 3.20e-06,
}


def gram_bar(dim, n):
    e = GRAM_ORACLE_ERR.get((dim, n))
    return GRAM_TOL if e is None else 4.0 * e


def gram_cases():
    """(dim, rows) of every Gramian case; each runs unweighted and weighted."""
    return ([(d, n) for d in GRAM_DIMS for n in GRAM_ROWS] +
            [(d, GRAM_BIG) for d in GRAM_BIG_DIMS] +
            [(d, n) for d in GRAM_WIDE_DIMS for n in GRAM_WIDE_ROWS])


def gram_rows(dim, n):
    """(X, w): fp32 N(0, 1) rows and U(0, 1) weights, every 7th exactly 0."""
    rng = np.random.default_rng(7919 * dim + n)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    w[3::7] = 0.0
    return X, w


def gram_err(G, G64):
    """max_ij |G - G64|_ij / sqrt(G64_ii G64_jj): the error on the
    Cauchy-Schwarz scale (0 / 0 = 0: a zero row of G64 has to be exact)."""
    d = np.sqrt(np.diag(G64))
    scale = np.outer(d, d)
    err = np.abs(G.astype(np.float64) - G64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    return float(q.max())
