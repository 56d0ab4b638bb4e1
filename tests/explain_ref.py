"""Float64 numpy reference of frecsys_explain, and its fixtures.

For the kinds IALS and WEIGHTED_U the projection of a history solves A x = b,

    A = s_G G + sum_j c_j y_j y_j^T + lambda I,   b = sum_j c_j y_j

(cg_ref.entity_terms is the table of s_G, c_j and lambda), so the score of a
target t splits exactly over the history entries:

    score(t) = v_t . x = sum_j contrib_j(t),   contrib_j(t) = c_j y_j^T A^-1 v_t.

It does not import the library.  CHUNK is the history rows one sweep of the
kernel's second pass takes (csrc/kernels.h kExplainChunk); GROUP the targets
of one substitution (kExplainGroup).
"""
import numpy as np

import cg_ref as C
import numpy_ref as R

TOL_ROW = C.TOL_ROW
N_OTHER = C.N_OTHER
DIMS = (8, 20, 64, 100, 200, 256)
KINDS = (C.KIND_IALS, C.KIND_U)
CHUNK = 256
GROUP = 32
TOPS = (1, 5, 32)
# (history length, targets) per row: every length seam against every group seam
ROWS = ((0, 5), (1, 1), (31, 31), (32, 32), (33, 33), (CHUNK - 1, 0), (CHUNK, 1),
        (CHUNK + 1, 70), (300, 7), (2 * CHUNK + 5, 33), (3, 5), (64, 3))


class Case(C.Case):
    """cg_ref.Case's tables and parameters with the histories of ROWS and a
    target list per row: its first targets are history items of the row, one
    target is repeated."""

    def __init__(self, kind, dim, side=C.SIDE_USER):
        super().__init__(kind, side, dim, len(ROWS))
        rng = np.random.default_rng(77 * dim + kind)
        hs = [h for h, _ in ROWS]
        self.ptr = np.concatenate([[0], np.cumsum(hs)]).astype(np.int64)
        self.col = np.concatenate(
            [rng.choice(N_OTHER, h, replace=False) for h in hs]).astype(np.int32)
        self.empty = [e for e, h in enumerate(hs) if h == 0]
        tg = []
        for e, (h, m) in enumerate(ROWS):
            t = rng.choice(N_OTHER, m, replace=True).astype(np.int32)
            inside = min(h, m // 3)
            t[:inside] = self.col[self.ptr[e]:self.ptr[e] + inside]
            if m >= 3:
                t[m - 1] = t[m // 2]  # a repeat
            tg.append(t)
        self.tgt_ptr = np.concatenate([[0], np.cumsum([len(t) for t in tg])]).astype(np.int64)
        self.tgt = np.concatenate(tg).astype(np.int32)

    def hist(self, e):
        return self.col[self.ptr[e]:self.ptr[e + 1]]

    def targets(self, e):
        return self.tgt[self.tgt_ptr[e]:self.tgt_ptr[e + 1]]

    def solve_kw(self):
        """Keyword arguments of Context.explain / solve_side for this case."""
        kw = dict(reg_exp=self.reg_exp)
        if self.kind == C.KIND_U:
            kw["entity_weight"] = self.omega
        return kw


def explain_entity(case, e, hist, targets, G=None, dtype=np.float64):
    """(contrib [h, m], score [m], x [d]) of entity e with history `hist`:
    the contributions of every history entry to every target, their column
    sums and the projection itself.  float64: np.linalg.solve; float32: the
    kernel's steps restated -- assemble, Cholesky, two substitutions, the
    second pass -- in float32 throughout."""
    if G is None:
        G = C.gram(case, dtype)
    d = case.dim
    V = case.X[targets].astype(dtype)
    if len(hist) == 0:
        return np.zeros((0, len(targets)), dtype), np.zeros(len(targets), dtype), np.zeros(d, dtype)
    sG, Y, c, bw, lam = C.entity_terms(case, e, hist, dtype)
    A = (sG * G + (Y * c[:, None]).T @ Y + lam * np.eye(d, dtype=dtype)).astype(dtype)
    b = Y.T @ bw
    if dtype == np.float64:
        W = np.linalg.solve(A, V.T)
        x = np.linalg.solve(A, b)
    else:
        L = np.linalg.cholesky(A)
        assert L.dtype == dtype
        W = np.linalg.solve(L.T, np.linalg.solve(L, V.T)).astype(dtype)
        x = np.linalg.solve(L.T, np.linalg.solve(L, b)).astype(dtype)
    contrib = (c[:, None] * (Y @ W)).astype(dtype)
    return contrib, contrib.sum(0), x


def explain_case(case, dtype=np.float64):
    """Per row (contrib, score, x) for the case's own histories and targets."""
    G = C.gram(case, dtype)
    return [explain_entity(case, e, case.hist(e), case.targets(e), G, dtype)
            for e in range(case.n_rows)]


def top_of(full, top):
    """(positions int64 [top], values [top]) of one pair's contributions: the
    `top` largest by (contribution descending, CSR position ascending),
    -1 / 0 behind the history length.  -0.0 orders as +0.0."""
    full = np.asarray(full)
    key = full + 0.0  # -0.0 -> +0.0
    order = np.lexsort((np.arange(len(full)), -key))[:top]
    pos = np.full(top, -1, np.int64)
    val = np.zeros(top, full.dtype)
    pos[:len(order)] = order
    val[:len(order)] = full[order]
    return pos, val


def pair_rel_err(contrib, ref):
    """Per pair: ||contrib - ref|| / ||ref|| over the history (columns)."""
    num = np.linalg.norm(np.asarray(contrib, np.float64) - ref, axis=0)
    return num / np.linalg.norm(ref, axis=0)


_cache = {}


def get_case(kind, dim):
    """The Case with its float64 reference (.ref), computed once per process."""
    if (kind, dim) not in _cache:
        c = Case(kind, dim)
        c.ref = explain_case(c)
        _cache[(kind, dim)] = c
    return _cache[(kind, dim)]
