"""Independent float64 numpy restatement of the reference's per-entity math
(dev-only checker for the C oracle; never used by the product).

Written from the reference sources, not from oracle/frecsys_oracle.c:
  iALS Project                ials.h:88-144
  ProjectU / ProjectU_eval    safer2.h:104-163, cvar_mf.h:182-229
  ProjectV (+ tail quirk)     safer2.h:166-221 (quirk :200-204)
  CVaR gradient steps         cvar_mf.h:88-180
  ComputeLoss                 ials.h:70-86, safer2.h:85-101
  SAFER2 smoothed quantile    safer2.h:598-742
"""
import math

import numpy as np


def ials(hist, X, G, reg, w):
    Xh = X[hist].astype(np.float64)
    A = w * G.astype(np.float64) + reg * np.eye(X.shape[1]) + Xh.T @ Xh
    return np.linalg.solve(A, Xh.sum(0))


def _quirk_rows(h):
    if h > 128 and h % 128:
        r = h % 128
        return np.arange(h - 128, h - r)
    return np.arange(0)


def assemble_u(hist, X, G, reg, w, omega):
    h = len(hist)
    Xh = X[hist].astype(np.float64)
    A = omega * (Xh.T @ Xh / h + w * G.astype(np.float64)) + reg * np.eye(X.shape[1])
    b = omega / h * Xh.sum(0)
    return A, b


def assemble_v(hist, X, G, reg, w, nu, quirk):
    h = len(hist)
    Xh = X[hist].astype(np.float64)
    nh = nu[hist].astype(np.float64)
    A = w * G.astype(np.float64) + (Xh * nh[:, None]).T @ Xh + reg * np.eye(X.shape[1])
    if quirk:
        q = _quirk_rows(h)
        if len(q):
            Xq = Xh[q]
            A += (Xq * nh[q][:, None]).T @ Xq
    b = (Xh * nh[:, None]).sum(0)
    return A, b


def project_u(hist, X, G, reg, w, omega):
    A, b = assemble_u(hist, X, G, reg, w, omega)
    return np.linalg.solve(A, b)


def project_v(hist, X, G, reg, w, nu, quirk):
    A, b = assemble_v(hist, X, G, reg, w, nu, quirk)
    return np.linalg.solve(A, b)


def _stale_upper(A, upper_vals):
    """Full matrix whose strict upper triangle holds `upper_vals` (the
    rank updates only wrote the lower part: SelfAdjointView<Lower>)."""
    L = np.tril(A)
    return L + np.triu(upper_vals, 1)


def cvar_u(hist, e, X, G, reg, w, eta, omega):
    A, b = assemble_u(hist, X, G, reg, w, omega)
    Af = _stale_upper(A, omega * w * G.astype(np.float64))
    return e - eta * (Af @ e - b)


def cvar_v(hist, e, X, G, reg, w, nu, eta, quirk):
    A, b = assemble_v(hist, X, G, reg, w, nu, quirk)
    Af = _stale_upper(A, w * G.astype(np.float64))
    return e - eta * (Af @ e - b)


# ---- whole-side drivers: one float64 half-step over every entity ----
# The Gramian is the float64 X^T X (or X^T diag(omega) X) of the fp32 rows,
# and lambda is the regularisation the models really pass (ials.h:310-315,
# safer2.h:418-432, cvar_mf.h:413-424). Scalars are taken at the fp32 value the
# library receives.  Rows with an empty history keep E's values.
def _f32(x):
    return float(np.float32(x))


def gram64(X, weights=None):
    X = X.astype(np.float64)
    if weights is None:
        return X.T @ X
    return X.T @ (X * weights.astype(np.float64)[:, None])


def _histories(ptr, col):
    for e in range(len(ptr) - 1):
        if ptr[e + 1] > ptr[e]:
            yield e, col[ptr[e]:ptr[e + 1]]


def ials_side(ptr, col, X, E, reg, w, reg_exp=1.0):
    reg, w, n_other = _f32(reg), _f32(w), X.shape[0]
    G = gram64(X)
    out = E.astype(np.float64)
    for e, hist in _histories(ptr, col):
        lam = reg * (len(hist) + w * n_other) ** _f32(reg_exp)
        out[e] = ials(hist, X, G, lam, w)
    return out


def project_u_side(ptr, col, X, E, reg, w, omega):
    reg, w = _f32(reg), _f32(w)
    lam = reg * (1.0 + w * X.shape[0])
    G = gram64(X)
    out = E.astype(np.float64)
    for e, hist in _histories(ptr, col):
        out[e] = project_u(hist, X, G, lam, w, float(omega[e]))
    return out


def project_v_side(ptr, col, X, E, reg, w, alpha, item_reg, nu, gram_weights, quirk):
    reg, w, alpha = _f32(reg), _f32(w), _f32(alpha)
    G = gram64(X, gram_weights)
    out = E.astype(np.float64)
    for e, hist in _histories(ptr, col):
        lam = reg * (float(item_reg[e]) + alpha * w * X.shape[0])
        out[e] = project_v(hist, X, G, lam, w, nu, quirk)
    return out


def cvar_u_side(ptr, col, X, E, reg, w, eta, omega):
    reg, w, eta = _f32(reg), _f32(w), _f32(eta)
    lam = reg * (1.0 + w * X.shape[0])
    G = gram64(X)
    out = E.astype(np.float64)
    for e, hist in _histories(ptr, col):
        out[e] = cvar_u(hist, out[e].copy(), X, G, lam, w, eta, float(omega[e]))
    return out


def cvar_v_side(ptr, col, X, E, reg, w, alpha, eta, item_reg, nu, gram_weights, quirk):
    reg, w, alpha, eta = _f32(reg), _f32(w), _f32(alpha), _f32(eta)
    G = gram64(X, gram_weights)
    out = E.astype(np.float64)
    for e, hist in _histories(ptr, col):
        lam = reg * (float(item_reg[e]) + alpha * w * X.shape[0])
        out[e] = cvar_v(hist, out[e].copy(), X, G, lam, w, nu, eta, quirk)
    return out


def user_loss(hist, u, X, G, beta, half):
    p = X[hist].astype(np.float64) @ u.astype(np.float64)
    l = np.mean((p - 1.0) ** 2) + beta * (u @ G.astype(np.float64) @ u)
    return l / 2 if half else l


# ---- SAFER2 smoothed quantile, float64 throughout ----
def _phi(u, h):
    return math.exp(-0.5 * (u / h) ** 2) / (h * math.sqrt(2 * math.pi))


def _Phi(u, h):
    return 0.5 * math.erfc(-(u / h) / math.sqrt(2))


def _gloss(u, h, alpha):
    ell = h * _phi(u, h) + (u / h) * (1 - 2 * _Phi(-u, h))
    return (h / 2) * ell + ((1 - alpha) - 0.5) * u


def _epan_k(u, h):
    uh = u / h
    return 0.75 * (1 - uh * uh) * (abs(uh) < 1) / h


def _epan_cdf(u, h):
    uh = u / h
    ins = abs(uh) <= 1
    pos = uh > 1
    return (h ** -3 / 4.0) * ((3 * u * h * h - u ** 3) + 2 * h ** 3) * ins + (1 - ins) * pos


def _epan_loss(u, h, alpha):
    uh = u / h
    ins = abs(uh) <= 1
    pos = uh > 1
    ell = (0.75 * uh ** 2 - uh ** 4 / 8 + 3 / 8) * ins + abs(uh) * pos
    return 0.5 * h * ell + ((1 - alpha) - 0.5) * u


def safer2_weight(loss, xi, bw, epan=False):
    r = loss - xi
    return 1 - (_epan_cdf(-r, bw) if epan else _Phi(-r, bw))


def _quantile(xi, losses, alpha, bw, epan):
    r = losses - xi
    if epan:
        g = (-(1 - alpha) + np.mean([_epan_cdf(-u, bw) for u in r])) / alpha
        H = np.mean([_epan_k(-u, bw) for u in r]) / alpha
        f = np.mean([_epan_loss(u, bw, alpha) for u in r]) / alpha
    else:
        g = (-(1 - alpha) + np.mean([_Phi(-u, bw) for u in r])) / alpha
        H = np.mean([_phi(-u, bw) for u in r]) / alpha
        f = np.mean([_gloss(u, bw, alpha) for u in r]) / alpha
    return f, g, H


def safer2_xi(losses, prev_xi, iters, alpha, bw, epan=False):
    xi = prev_xi
    for _ in range(iters):
        f0, g0, H = _quantile(xi, losses, alpha, bw, epan)
        d = g0 / H
        gamma = 1.0
        x = xi - gamma * d
        for _ in range(32):
            fx, gx, _ = _quantile(x, losses, alpha, bw, epan)
            if fx > f0 + 1e-4 * gamma * gx * (-d):
                gamma *= 0.5
                x = xi - gamma * d
            else:
                break
        xi = xi - gamma * d
    return xi


# ---- the kernels around the solve (tests/aux_data.py), float64 throughout ----
def user_loss_side(ptr, col, U, V, G64, beta, half):
    """ComputeUserLoss over one side: l_e of every row with a history, 0 for
    the empty ones.  G64: the float64 Gramian of V (gram64); beta at the fp32
    value the library receives."""
    beta = _f32(beta)
    out = np.zeros(len(ptr) - 1)
    for e, hist in _histories(ptr, col):
        out[e] = user_loss(hist, U[e], V, G64, beta, half)
    return out


def train_stats64(up, uc, U, V):
    """(observed, unobserved, ||U_r||^2, ||V_r||^2): the parts of
    ComputeLosses (ials.h:226-305): sum over the observed pairs of (u.v - 1)^2
    and sum_ij (U^T U)_ij (V^T V)_ij."""
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    rows = np.repeat(np.arange(len(up) - 1), np.diff(up))
    pred = np.einsum("ij,ij->i", U64[rows], V64[uc])
    obs = float(np.sum((pred - 1.0) ** 2))
    unobs = float(np.sum(gram64(U) * gram64(V)))
    return obs, unobs, np.sum(U64 ** 2, axis=1), np.sum(V64 ** 2, axis=1)


def topk64(Ue, V, ep, ec, k):
    """(S, top): the float64 scores with every history item at -inf, and per
    row the k first items by (score descending, item id ascending) -- so the
    excluded items come after every free one, by ascending id."""
    S = Ue.astype(np.float64) @ V.astype(np.float64).T
    for r in range(len(ep) - 1):
        S[r, ec[ep[r]:ep[r + 1]]] = -np.inf
    ids = np.broadcast_to(np.arange(S.shape[1]), S.shape)
    order = np.lexsort((ids, -S), axis=1)
    return S, order[:, :k].astype(np.int32)


def topk_close_rows(S, k, rtol=2e-6):
    """Rows of S (topk64) whose ranking fp32 scores cannot be asked to
    reproduce exactly: two adjacent listed scores, or the k-th and the
    (k+1)-th, closer than rtol * max|S|.  Excluded items (-inf) tie exactly
    and are ordered by id, which is exact in any precision: they never flag."""
    tol = rtol * np.abs(S[np.isfinite(S)]).max() if np.isfinite(S).any() else 0.0
    srt = -np.sort(-S, axis=1)[:, :k + 1]
    with np.errstate(invalid="ignore"):
        gap = srt[:, :-1] - srt[:, 1:]
    fin = np.isfinite(srt[:, :-1]) & np.isfinite(srt[:, 1:])
    return np.any(fin & (gap < tol), axis=1), tol
