"""Float64 numpy restatement of one iALS++ / SAFER2++ block step, and the
cases test_pp_seam_cpu.py / test_pp_seam_gpu.py run it on.

Written from the formulas in the header comment of csrc/pp.hip and in
oracle/frecsys_oracle.c pp_step_row; it does not import the library.  For an
entity with history H (h = |H|, repeated ids are repeated tuples), block
columns [s, e), x_j = the block columns of the other side's row j, u = the
entity's full row, p_j = the current prediction of the tuple,
Gl = Xw[:, s:e]^T X[:, s:e] and Glg = Xw[:, s:e]^T X (Xw = X, or X scaled per
row by the Gramian weights omega in the V kind):

    IALS        lam = reg (h + w n_other)^reg_exp
                A = w Gl + sum x_j x_j^T + lam I
                r = sum x_j (p_j - 1) + w Glg u + lam u[s:e]
    WEIGHTED_U  lam = reg (1 + w n_other), om = the entity's weight
                A = (sum x_j x_j^T / h + w Gl) om + lam I
                r = (sum x_j (p_j - 1)) om / h + w om Glg u + lam u[s:e]
    WEIGHTED_V  lam = reg (entity_reg + alpha w n_other)
                A = w Gl + sum nu_j x_j x_j^T + lam I
                r = sum nu_j x_j (p_j - 1) + w Glg u + lam u[s:e]

    delta = -A^-1 r;  u[s:e] += delta;  p_j += delta . x_j for every tuple;
    residual = sum over entities of |delta|^2.

Empty histories are untouched, and the block step has no tail quirk.

The cases stand on seam_data.seam_case(key, dim) with its weights unchanged.
The rating index of a CSR entry is the file position of its tuple: with the
file-order pair list of seam_data._pairs, the stable argsort of the user
column (user CSR) and of the item column (item CSR).  In the as_items
orientation the user side's index is a non-identity permutation too.

Error measures, per live entity (the denominators include the step itself,
so they stay finite where the new block is about 0 -- an omega = 0 entity has
A = lam I, r = lam u and a new block that is 0 only up to rounding):

    block       ||blk - ref_blk|| / max(||ref_blk||, ||ref_delta||)
    prediction  ||pred_e - ref_pred_e|| / max(||ref_pred_e||, ||ref_dpred_e||)

the first over the block columns only, the second over the entity's tuples.
"""
import types

import numpy as np

import seam_data as S

TOL = 1e-4               # the project's row bar
ORACLE_CAP = 0.25 * TOL  # the fp32 restatement's own share of it

KEYS = ("ials_user", "ials_item", "ials_exp0", "weighted_u", "weighted_v_plain")
PADDED = {8: 8, 20: 32, 100: 128, 200: 224, 256: 256, 500: 512, 1000: 1024}  # dim: Dp
DIMS = tuple(PADDED)
WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
HISTORY_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65)

# The same list for every key.  Width-1 blocks [19,20) at d = 20, [255,256)
# at d = 256 and [999,1000) at d = 1000 are not in it: there the fp32 oracle
# itself is 3e-5..5e-5 from float64 with ials_exp0 (cancellation in a
# one-term right-hand side), over ORACLE_CAP.
BLOCKS = {
    8: ((0, 8), (0, 1), (7, 8), (2, 7)),
    20: ((0, 20), (18, 20)),
    100: ((0, 31), (31, 63), (67, 100), (0, 64), (35, 100), (5, 100), (4, 100), (3, 100)),
    200: ((0, 97), (72, 200), (73, 200), (198, 200)),
    256: ((0, 128), (128, 256), (96, 161), (193, 256), (254, 256)),
    500: ((372, 500), (404, 500), (0, 96)),
    1000: ((905, 1000), (0, 128), (872, 1000), (500, 564), (998, 1000)),
}
CASES = [(k, d, b) for d in DIMS for k in KEYS for b in BLOCKS[d]]
TWO_STEP = ((0, 65), (65, 100))  # at d = 100
TWO_STEP_KEYS = ("ials_user", "weighted_v_plain")


def case_id(p):
    key, dim, (s, e) = p
    return f"{key}-{dim}-{s}_{e}"


def tile_count(width):
    """TB of pp_block_kernel<TB>: 32-column tiles of the padded block."""
    return (width + 31) // 32


def check_coverage(blocks=BLOCKS, padded=PADDED):
    """The conditions the block list must meet (the lower and upper width of
    every TB, one element on either side of every 32-column tile, unaligned
    starts, ends at dim with and without padding behind them)."""
    every = [(d, s, e) for d, bl in blocks.items() for s, e in bl]
    for d, s, e in every:
        assert 0 <= s < e <= d and e - s <= 128, (d, s, e)
    widths = {e - s for _, s, e in every}
    assert set(WIDTHS) <= widths, sorted(set(WIDTHS) - widths)
    for tb in (1, 2, 3, 4):
        mine = [(d, s, e) for d, s, e in every if tile_count(e - s) == tb]
        assert any(s % 32 for _, s, _ in mine), tb
        assert any(e == d for d, _, e in mine), tb
    assert any(e == d and d < padded[d] for d, _, e in every)


def rating_indices(c):
    """(urix, irix) of seam case c: the file position of every CSR entry."""
    ent, oth = S._pairs(S.seam_data())
    users_file, items_file = (ent, oth) if c.seam == "user" else (oth, ent)
    urix = np.argsort(users_file, kind="stable").astype(np.int32)
    irix = np.argsort(items_file, kind="stable").astype(np.int32)
    np.testing.assert_array_equal(c.uc, items_file[urix])
    np.testing.assert_array_equal(c.ic, users_file[irix])
    return urix, irix


_cases, _pred0, _refs, _oracle_pred0, _oracle = {}, {}, {}, {}, {}


def pp_case(key, dim):
    """seam_case(key, dim) plus the rating indices; rix is the solved side's."""
    if (key, dim) not in _cases:
        c = S.seam_case(key, dim)
        urix, irix = rating_indices(c)
        p = types.SimpleNamespace(c=c, key=key, dim=dim, urix=urix, irix=irix,
                                  rix=urix if c.seam == "user" else irix, nnz=len(c.uc),
                                  live=np.nonzero(c.h > 0)[0])
        _cases[key, dim] = p
    return _cases[key, dim]


def predict(ptr, col, rix, X, E, with_abs=False):
    """float64 PredictDataset: pred[rix[k]] = X[col[k]] . E[row]; with_abs
    also returns sum_i |x_i u_i| per entry (for a dot-product bound)."""
    X = np.asarray(X, np.float64)
    E = np.asarray(E, np.float64)
    pred = np.zeros(len(col))
    mag = np.zeros(len(col))
    for r in range(len(ptr) - 1):
        p0, p1 = ptr[r], ptr[r + 1]
        if p1 > p0:
            pred[rix[p0:p1]] = X[col[p0:p1]] @ E[r]
            if with_abs:
                mag[rix[p0:p1]] = np.abs(X[col[p0:p1]]) @ np.abs(E[r])
    return (pred, mag) if with_abs else pred


def _f32(x):
    """A scalar as the fp32 the library and the oracle receive."""
    return float(np.float32(x))


def entity_lambda(c, ent, h, reg=None):
    reg = _f32(c.reg if reg is None else reg)
    w = _f32(c.w)
    if c.kind == 0:
        return reg * (h + w * c.n_other) ** _f32(c.reg_exp)
    if c.kind == 1:
        return reg * (1.0 + w * c.n_other)
    return reg * (float(c.entity_reg[ent]) + _f32(c.alpha) * w * c.n_other)


def _local_gramians(c, s, e):
    X = c.X.astype(np.float64)
    Xw = X[:, s:e] * c.gram_weights.astype(np.float64)[:, None] if c.kind == 2 else X[:, s:e]
    return X, Xw.T @ X[:, s:e], Xw.T @ X


def _system(c, ent, s, e, X, Gl, Glg, E, pred, rix, reg):
    """(A, r, x, idx) of entity ent on block [s, e)."""
    p0, p1 = c.ptr[ent], c.ptr[ent + 1]
    h = int(p1 - p0)
    hist, idx = c.col[p0:p1], rix[p0:p1]
    x = X[hist, s:e]
    res = pred[idx] - 1.0
    u = E[ent]
    w = _f32(c.w)
    lam = entity_lambda(c, ent, h, reg)
    eye = np.eye(e - s)
    if c.kind == 0:
        A = w * Gl + x.T @ x + lam * eye
        r = x.T @ res + w * (Glg @ u) + lam * u[s:e]
    elif c.kind == 1:
        om = float(c.entity_weight[ent])
        A = (x.T @ x / h + w * Gl) * om + lam * eye
        r = (x.T @ res) * om / h + w * om * (Glg @ u) + lam * u[s:e]
    else:
        nu = c.other_weight.astype(np.float64)[hist]
        A = w * Gl + (x * nu[:, None]).T @ x + lam * eye
        r = x.T @ (nu * res) + w * (Glg @ u) + lam * u[s:e]
    return A, r, x, idx


def block_step(c, rix, E, pred, s, e, reg=None):
    """One float64 block step of case c on columns [s, e) from rows E and
    predictions pred (both float64, not modified).  Returns the new rows, the
    new predictions, delta [n, e - s], the change of every prediction and the
    residual."""
    X, Gl, Glg = _local_gramians(c, s, e)
    E, pred = E.copy(), pred.copy()
    delta = np.zeros((len(c.h), e - s))
    dpred = np.zeros(len(pred))
    for ent in np.nonzero(c.h > 0)[0]:
        A, r, x, idx = _system(c, ent, s, e, X, Gl, Glg, E, pred, rix, reg)
        d = -np.linalg.solve(A, r)
        E[ent, s:e] += d
        dpred[idx] = x @ d  # rating indices are distinct: repeats are tuples of their own
        delta[ent] = d
    return E, pred + dpred, delta, dpred, float((delta ** 2).sum())


def min_eigenvalues(p, s, e, reg):
    """Smallest eigenvalue of every live entity's block matrix with `reg`."""
    c = p.c
    X, Gl, Glg = _local_gramians(c, s, e)
    E, pred = c.E.astype(np.float64), pred0(p)
    return np.array([np.linalg.eigvalsh(_system(c, ent, s, e, X, Gl, Glg, E, pred, p.rix, reg)[0])[0]
                     for ent in p.live])


def pred0(p):
    """float64 predictions of the start embeddings (PredictDataset over the
    user CSR), and sum |x_i u_i| per entry."""
    if (p.key, p.dim) not in _pred0:
        c = p.c
        out = predict(c.up, c.uc, p.urix, c.V, c.U, with_abs=True)
        for a in out:
            a.setflags(write=False)
        _pred0[p.key, p.dim] = out
    return _pred0[p.key, p.dim][0]


def pred0_magnitude(p):
    pred0(p)
    return _pred0[p.key, p.dim][1]


def reference(key, dim, blocks):
    """The float64 steps of case (key, dim) on `blocks` (one (s, e) or a
    sequence of them, each consuming the predictions of the one before), from
    the fixture's start rows: a list of SimpleNamespace(s, e, E, pred, delta,
    dpred, residual), computed once."""
    blocks = _seq(blocks)
    k = (key, dim, blocks)
    if k not in _refs:
        p = pp_case(key, dim)
        E, pred = p.c.E.astype(np.float64), pred0(p)
        out = []
        for s, e in blocks:
            E, pred, delta, dpred, res = block_step(p.c, p.rix, E, pred, s, e)
            for a in (E, pred, delta, dpred):
                a.setflags(write=False)
            out.append(types.SimpleNamespace(s=s, e=e, E=E, pred=pred, delta=delta, dpred=dpred,
                                             residual=res))
        _refs[k] = out
    return _refs[k]


def oracle_steps(key, dim, blocks):
    """The fp32 C oracle on the same sequence: a list of SimpleNamespace(rc, E,
    pred, residual) (oracle.pp_predict once, then oracle.pp_step per block)."""
    blocks = _seq(blocks)
    k = (key, dim, blocks)
    if k not in _oracle:
        import oracle as O
        p = pp_case(key, dim)
        c = p.c
        if (key, dim) not in _oracle_pred0:
            pr = np.zeros(p.nnz, np.float32)
            O.pp_predict(c.up, c.uc, p.urix, c.V, c.U, pr)
            pr.setflags(write=False)
            _oracle_pred0[key, dim] = pr
        pred = _oracle_pred0[key, dim].copy()
        E = c.E.copy()
        out = []
        for s, e in blocks:
            rc, res = O.pp_step(c.ptr, c.col, p.rix, c.X, E, pred, s, e, c.reg, c.w,
                                reg_exp=getattr(c, "reg_exp", 1.0), kind=c.kind,
                                alpha=getattr(c, "alpha", 0.0), entity_weight=c.entity_weight,
                                entity_reg=c.entity_reg, other_weight=c.other_weight,
                                gram_w=c.gram_weights)
            out.append(types.SimpleNamespace(rc=rc, E=E.copy(), pred=pred.copy(), residual=res))
        _oracle[k] = out
    return _oracle[k]


def oracle_pred0(key, dim):
    oracle_steps(key, dim, BLOCKS[dim][0])
    return _oracle_pred0[key, dim]


def _seq(blocks):
    blocks = tuple(blocks)
    return (blocks,) if isinstance(blocks[0], (int, np.integer)) else tuple(map(tuple, blocks))


def block_errors(p, ref, E):
    """Block error of every live entity (in the order of p.live)."""
    s, e = ref.s, ref.e
    live = p.live
    num = np.linalg.norm(E[live, s:e].astype(np.float64) - ref.E[live, s:e], axis=1)
    den = np.maximum(np.linalg.norm(ref.E[live, s:e], axis=1),
                     np.linalg.norm(ref.delta[live], axis=1))
    return num / den


def pred_errors(p, ref, pred):
    """Prediction error of every live entity over its own tuples."""
    c = p.c
    out = np.zeros(len(p.live))
    diff = pred.astype(np.float64) - ref.pred
    for i, ent in enumerate(p.live):
        idx = p.rix[c.ptr[ent]:c.ptr[ent + 1]]
        den = max(np.linalg.norm(ref.pred[idx]), np.linalg.norm(ref.dpred[idx]))
        out[i] = np.linalg.norm(diff[idx]) / den
    return out


def offenders(p, err, bar):
    """(h, label, error) of every live entity not under the bar."""
    c = p.c
    return [(int(c.h[ent]), c.labels[ent], float(x)) for ent, x in zip(p.live, err) if not x < bar]


def worst(p, err):
    """(error, h, label) of the worst live entity."""
    i = int(np.argmax(err))
    ent = p.live[i]
    return float(err[i]), int(p.c.h[ent]), p.c.labels[ent]
