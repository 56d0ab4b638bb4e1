"""Float64 numpy conjugate gradients for the --use_cg path, and its fixtures.

Written from the reference headers (ials.h:133-139, safer2.h:152-157,
210-215: Eigen::ConjugateGradient<MatrixXf, Lower> with its default
DiagonalPreconditioner, zero initial guess) and Eigen's conjugate_gradient
recurrence; it does not import the library.  Matrix-free:

    A p     = s_G (G p) + sum_j c_j y_j (y_j . p) + lambda p
    diag(A) = s_G G_ii  + sum_j c_j y_ji^2        + lambda

    kind        s_G       c_j       b
    IALS        w         1         sum y_j
    WEIGHTED_U  omega w   omega/h   (omega/h) sum y_j
    WEIGHTED_V  w         nu_j      sum nu_j y_j   (G omega-weighted; with the
                tail quirk the rows numpy_ref._quirk_rows names are in c_j
                twice and in b once)

The float64 direct solve of the same systems comes from tests/numpy_ref.py.
`dtype=np.float32` runs the same recurrence in float32 (the CPU tests bound
the rounding of the recurrence itself on every fixture the GPU tests use).
"""
import numpy as np

import numpy_ref as R

KIND_IALS, KIND_U, KIND_V = 0, 1, 2
SIDE_USER, SIDE_ITEM, SIDE_EVAL = 0, 1, 2
TOL_ROW = 1e-4
N_OTHER = 600
DIMS = (8, 20, 64, 100, 200, 256)
CAPS = (1, 2, 5)


def padded_dim(d):
    return d if d in (8, 16) else (16 if d < 16 else -(-d // 32) * 32)


def row_chunk(d):
    """History rows one wave of the kernel keeps in flight: 8 passes of
    64 / GP rows, GP = the power of two >= Dp / 4 (at least 2)."""
    gp = 2
    while gp < padded_dim(d) // 4:
        gp *= 2
    return 8 * (64 // gp)


COOP_ROWS = 256  # longer histories are streamed by all four waves of a workgroup


def history_lengths(d):
    c = row_chunk(d)
    return [1, 3, 64, 129, 300, c - 1, c, c + 1, COOP_ROWS, COOP_ROWS + 1]


class Case:
    """One solve of `n_rows` entities of `side` against N_OTHER other rows."""

    def __init__(self, kind, side, dim, n_rows, quirk=False, seed=0):
        rng = np.random.default_rng(1000 * dim + 10 * n_rows + 3 * kind + side + seed)
        self.kind, self.side, self.dim, self.n_rows, self.quirk = kind, side, dim, n_rows, quirk
        self.n_other = N_OTHER
        self.X = (rng.standard_normal((N_OTHER, dim)) / np.sqrt(dim)).astype(np.float32)
        self.E0 = (rng.standard_normal((n_rows, dim)) / np.sqrt(dim)).astype(np.float32)
        lens = history_lengths(dim)
        if n_rows == 1:
            hs = [300]
        else:
            hs = [lens[i % len(lens)] for i in range(n_rows)]
            hs[7 % n_rows] = 0 if n_rows > 8 else hs[7 % n_rows]
            hs[n_rows - 2] = 0
            if kind == KIND_V:
                hs[0] = 300  # the tail quirk's h
        self.empty = [e for e, h in enumerate(hs) if h == 0]
        self.ptr = np.concatenate([[0], np.cumsum(hs)]).astype(np.int64)
        self.col = np.concatenate(
            [rng.choice(N_OTHER, h, replace=False) for h in hs] + [np.zeros(0, np.int64)]
        ).astype(np.int32)
        self.reg, self.w, self.reg_exp, self.alpha = 0.003, 0.1, 1.0, 0.3
        # WEIGHTED_U: log-uniform over [2e-3, 1] (the smoothed tail weights reach
        # down to 0), so cond(A) -- and the iteration count at a tolerance --
        # differs between the rows
        self.omega = np.exp(rng.uniform(np.log(2e-3), 0.0, n_rows)).astype(np.float32)
        self.item_reg = rng.uniform(0.5, 1.5, n_rows).astype(np.float32)     # WEIGHTED_V
        self.omega_other = rng.uniform(0.05, 1.0, N_OTHER).astype(np.float32)
        self.nu = (self.omega_other / rng.integers(2, 40, N_OTHER)).astype(np.float32)
        self.gram_weights = self.omega_other if kind == KIND_V else None

    def histories(self):
        for e in range(self.n_rows):
            if self.ptr[e + 1] > self.ptr[e]:
                yield e, self.col[self.ptr[e]:self.ptr[e + 1]]

    def lam(self, e, h):
        reg, w, alpha = R._f32(self.reg), R._f32(self.w), R._f32(self.alpha)
        if self.kind == KIND_IALS:
            return reg * (h + w * self.n_other) ** R._f32(self.reg_exp)
        if self.kind == KIND_U:
            return reg * (1.0 + w * self.n_other)
        return reg * (float(self.item_reg[e]) + alpha * w * self.n_other)


def entity_terms(case, e, hist, dtype):
    """(s_G, Y, c, bw, lambda): the operator terms of one entity."""
    h = len(hist)
    w = R._f32(case.w)
    Y = case.X[hist].astype(dtype)
    if case.kind == KIND_IALS:
        sG, c = w, np.ones(h, dtype)
        bw = c
    elif case.kind == KIND_U:
        om = float(case.omega[e])
        sG, c = om * w, np.full(h, om / h, dtype)
        bw = c
    else:
        sG, c = w, case.nu[hist].astype(dtype)
        bw = c
        if case.quirk:
            q = R._quirk_rows(h)
            if len(q):
                Y = np.concatenate([Y, Y[q]])
                bw = np.concatenate([c, np.zeros(len(q), dtype)])
                c = np.concatenate([c, c[q]])
    return dtype(sG), Y, c.astype(dtype), bw.astype(dtype), dtype(case.lam(e, h))


def cg_entity(G, sG, Y, c, bw, lam, max_it, tol, dtype, snaps=()):
    """Eigen's conjugate_gradient with the Jacobi preconditioner from x = 0.
    Returns (x, i, {cap: iterate after `cap` iterations for cap in snaps})."""
    tiny = dtype(np.finfo(np.float32).tiny)
    d = G.shape[0]

    def A(p):
        return sG * (G @ p) + Y.T @ (c * (Y @ p)) + lam * p

    out = {}
    b = Y.T @ bw
    x = np.zeros(d, dtype)
    bn2 = b @ b
    if bn2 == 0:
        return x, 0, {s: x.copy() for s in snaps}
    thr = max(dtype(tol) * dtype(tol) * bn2, tiny)
    r = b.copy()
    if r @ r < thr:
        return x, 0, {s: x.copy() for s in snaps}
    diag = sG * np.diag(G) + (c[:, None] * Y * Y).sum(0) + lam
    inv = np.where(diag != 0, 1 / np.where(diag != 0, diag, 1), 1).astype(dtype)
    p = r * inv
    rho = r @ p
    i = 0
    while i < max_it:
        t = A(p)
        alpha = rho / (p @ t)
        x = x + alpha * p
        r = r - alpha * t
        if i + 1 in snaps:
            out[i + 1] = x.copy()
        if r @ r < thr:
            break
        z = r * inv
        rho1 = r @ z
        p = z + (rho1 / rho) * p
        rho = rho1
        i += 1
    for s in snaps:
        out.setdefault(s, x.copy())
    return x, i, out


def gram(case, dtype):
    X = case.X.astype(dtype)
    if case.gram_weights is None:
        return X.T @ X
    return X.T @ (X * case.gram_weights.astype(dtype)[:, None])


def cg_side(case, max_it, tol, dtype=np.float64, snaps=()):
    """(out [n_rows, d], iters [n_rows], {cap: out at that cap}): rows with an
    empty history keep E0 and -1."""
    G = gram(case, dtype)
    out = case.E0.astype(dtype)
    its = np.full(case.n_rows, -1, np.int32)
    at = {s: case.E0.astype(dtype) for s in snaps}
    for e, hist in case.histories():
        x, i, sn = cg_entity(G, *entity_terms(case, e, hist, dtype), max_it, tol, dtype, snaps)
        out[e], its[e] = x, i
        for s in snaps:
            at[s][e] = sn[s]
    return out, its, at


def direct_side(case):
    """The float64 direct solve of every entity (tests/numpy_ref.py)."""
    G = R.gram64(case.X, case.gram_weights)
    w = R._f32(case.w)
    out = case.E0.astype(np.float64)
    for e, hist in case.histories():
        lam = case.lam(e, len(hist))
        if case.kind == KIND_IALS:
            out[e] = R.ials(hist, case.X, G, lam, w)
        elif case.kind == KIND_U:
            out[e] = R.project_u(hist, case.X, G, lam, w, float(case.omega[e]))
        else:
            out[e] = R.project_v(hist, case.X, G, lam, w, case.nu, case.quirk)
    return out


def residual_side(case, x):
    """True float64 relative residual ||b - A x|| / ||b|| per row (0 for empty)."""
    G = gram(case, np.float64)
    res = np.zeros(case.n_rows)
    for e, hist in case.histories():
        sG, Y, c, bw, lam = entity_terms(case, e, hist, np.float64)
        xe = x[e].astype(np.float64)
        b = Y.T @ bw
        Ax = sG * (G @ xe) + Y.T @ (c * (Y @ xe)) + lam * xe
        res[e] = np.linalg.norm(b - Ax) / np.linalg.norm(b)
    return res


def gpu_cases():
    """Every fixture tests/test_cg_gpu.py solves: (id, Case arguments)."""
    out = []
    for d in DIMS:
        for n in (1, 33, 70):
            out.append((f"ials-user-d{d}-n{n}", (KIND_IALS, SIDE_USER, d, n, False)))
        out.append((f"ials-item-d{d}-n70", (KIND_IALS, SIDE_ITEM, d, 70, False)))
        out.append((f"u-user-d{d}-n33", (KIND_U, SIDE_USER, d, 33, False)))
        out.append((f"v-item-d{d}-n33", (KIND_V, SIDE_ITEM, d, 33, False)))
        out.append((f"vquirk-item-d{d}-n70", (KIND_V, SIDE_ITEM, d, 70, True)))
    return out


_cache = {}


def get_case(args):
    """The Case of `args` with its references, computed once per process:
    .trunc {cap: float64 iterate}, .conv (cg at 100 iterations, tolerance
    1e-10), .direct."""
    if args not in _cache:
        c = Case(*args)
        _, _, c.trunc = cg_side(c, max(CAPS), 0.0, np.float64, CAPS)
        c.conv, c.conv_iters, _ = cg_side(c, 100, 1e-10, np.float64)
        c.direct = direct_side(c)
        _cache[args] = c
    return _cache[args]
