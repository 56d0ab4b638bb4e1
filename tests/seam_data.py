"""One deterministic fixture that puts an entity on every history-length seam
of the solve paths (train.hip plan_side queue split, solve.hip slabs,
dual.hip buckets), and the float64 / oracle references of a half-step on it.

The "seam entities" are the solved side: S histories over N_OTHER = 704 rows
of the other side.  as_users() / as_items() give the usual
(n_users, n_items, up, uc, ip, ic) with the seam entities as the users or as
the items (the transposed orientation), both CSRs built from one file-order
pair list.

  edges    h = 1, 2, then 32 t - 1, 32 t, 32 t + 1 for t = 1..16, then 639, 640:
           the wave kernels (TH <= 2), every dual_solve_kernel<TH> with zero
           and with 31 padding rows, the 224 | 225 and 256 | 257 crossovers,
           the user side's 320 | 321 at Dp = 512, the wide bucket's 512 | 513,
           d space above it; under the ProjectV tail quirk (h_eff = h + 128 -
           h % 128) 129 and 255 -> 256, 257 and 383 -> 384, 385 and 511 ->
           512, 513 and 639 -> 640
  extreme  [0], [n-1], [0, n-1], the last 32 ids, the last 33 ids
  repeats  40 distinct ids + 3 repeats of one + 21 of another (h = 64);
           20 distinct + the first 13 again (h = 33); 150 distinct + the
           first 107 again (h = 257).  dataset.h keeps repeated (user, item)
           lines as repeated rows, so these are legal input.  (Not one row
           for the whole history: 64 copies of one row are ill-conditioned
           enough that fp32 itself is 4.7e-4 from float64 at d = 1000.)
  idle     empty histories at index 0, in the middle and at index S - 1
  filler   40 entities with h drawn from [3, 200)
  nu0      one entity whose history holds only rows with nu = 0

Zero weights: omega = 0 for every 11th seam entity (index % 11 == 6: h = 63,
161, 288, 415, 513 and fillers) in the U kinds; nu = 0 for every 9th row of
the other side (index % 9 == 4, so neither the first nor the last row) in the
V kinds.
"""
import types

import numpy as np

import numpy_ref as R

N_OTHER = 704
EDGE_LENGTHS = (1, 2) + tuple(32 * t + k for t in range(1, 17) for k in (-1, 0, 1)) + (639, 640)
QUIRK_HEFF = {129: 256, 255: 256, 257: 384, 383: 384, 385: 512, 511: 512, 513: 640, 639: 640}
OMEGA_ZERO = (6, 11)  # seam entity e has omega = 0 when e % 11 == 6
NU_ZERO = (4, 9)      # other-side row r has nu = 0 when r % 9 == 4
SEED = 29


def h_eff(h, quirk):
    """Rows the assembly reads: the ProjectV tail quirk re-reads the rows of
    the last full 128-block (safer2.h:200-204)."""
    h = np.asarray(h)
    return np.where(bool(quirk) & (h > 128) & (h % 128 != 0), h + 128 - h % 128, h)


def make_seam_data(seed=SEED):
    """SimpleNamespace(hists, labels, n_other): hists[e] is entity e's history
    in file order (int64 ids < n_other), labels[e] says why it is there."""
    rng = np.random.default_rng(seed)
    n = N_OTHER
    hists, labels = [], []

    def add(label, hist):
        hists.append(np.asarray(hist, np.int64))
        labels.append(label)

    def draw(h):
        return rng.permutation(n)[:h]

    add("idle", [])
    for h in EDGE_LENGTHS:
        add(f"edge{h}", draw(h))
    add("first", [0])
    add("last", [n - 1])
    add("first_last", [0, n - 1])
    add("last32", np.arange(n - 32, n))
    add("last33", np.arange(n - 33, n))
    a = draw(40)
    add("repeat64", np.concatenate([a, np.repeat(a[7], 3), np.repeat(a[23], 21)]))
    a = draw(20)
    add("repeat33", np.concatenate([a, a[:13]]))
    a = draw(150)
    add("repeat257", np.concatenate([a, a[:107]]))
    add("idle", [])
    for _ in range(40):
        add("filler", draw(int(rng.integers(3, 200))))
    add("nu0", rng.permutation(np.arange(NU_ZERO[0], n, NU_ZERO[1]))[:12])
    add("idle", [])
    return types.SimpleNamespace(hists=hists, labels=labels, n_other=n)


def _pairs(sd):
    ent = np.concatenate([np.full(len(h), e, np.int64) for e, h in enumerate(sd.hists)])
    return ent, np.concatenate(sd.hists)


def as_users(sd):
    from frecsys_hip.data import _csr_from_pairs
    ent, oth = _pairs(sd)
    up, uc = _csr_from_pairs(ent, oth, len(sd.hists))
    ip, ic = _csr_from_pairs(oth, ent, sd.n_other)
    return len(sd.hists), sd.n_other, up, uc, ip, ic


def as_items(sd):
    from frecsys_hip.data import _csr_from_pairs
    ent, oth = _pairs(sd)
    up, uc = _csr_from_pairs(oth, ent, sd.n_other)
    ip, ic = _csr_from_pairs(ent, oth, len(sd.hists))
    return sd.n_other, len(sd.hists), up, uc, ip, ic


# ---- the half-steps run on it ----
# kind: the oracle's / the library's kind number (iALS, ProjectU, ProjectV,
# CVaR U step, CVaR V step); seam: which side the seam entities are.
# reg / w / alpha as in test_parity_gpu.py.
KINDS = {
    "ials_user": dict(kind=0, seam="user", reg=0.003, w=0.1, reg_exp=1.0),
    "ials_item": dict(kind=0, seam="item", reg=0.003, w=0.1, reg_exp=1.0),
    "ials_exp0": dict(kind=0, seam="user", reg=0.003, w=0.1, reg_exp=0.0),
    "weighted_u": dict(kind=1, seam="user", reg=0.004, w=0.004),
    "weighted_v_quirk": dict(kind=2, seam="item", reg=0.004, w=0.004, alpha=0.3, quirk=True),
    "weighted_v_plain": dict(kind=2, seam="item", reg=0.004, w=0.004, alpha=0.3, quirk=False),
    "cvar_u": dict(kind=3, seam="user", reg=0.002, w=0.008, eta=0.4),
    "cvar_v": dict(kind=4, seam="item", reg=0.002, w=0.008, alpha=0.3, eta=0.4, quirk=True),
}

_cases, _refs, _oracle = {}, {}, {}
_data = {}


def seam_data():
    if not _data:
        sd = make_seam_data()
        _data.update(sd=sd, user=as_users(sd), item=as_items(sd))
    return _data["sd"]


def seam_case(key, dim):
    """Everything one half-step needs: the CSRs, the fp32 embeddings of
    oracle.init_embeddings(1, 0.1), the weights, and the solved side's view
    (ptr, col, X = the other side's rows, E = the solved side's rows)."""
    if (key, dim) not in _cases:
        sd = seam_data()
        _cases[key, dim] = build_case(key, dim, sd.labels, _data[KINDS[key]["seam"]], "seam")
    return _cases[key, dim]


def build_case(key, dim, labels, oriented, fixture):
    """seam_case for any fixture: `oriented` is as_users(sd) or as_items(sd)
    of the data whose solved-side labels are `labels`, matching the seam side
    of KINDS[key]; `fixture` names the data in the reference caches."""
    import oracle as O
    p = KINDS[key]
    nu, ni, up, uc, ip, ic = oriented
    U, V = O.init_embeddings(1, 0.1, dim, nu, ni)
    c = types.SimpleNamespace(key=key, dim=dim, fixture=fixture, labels=labels, nu=nu, ni=ni,
                              up=up, uc=uc, ip=ip, ic=ic, U=U, V=V, entity_weight=None,
                              entity_reg=None, other_weight=None, gram_weights=None, **p)
    c.quirk = bool(p.get("quirk", True))
    if c.seam == "user":
        c.ptr, c.col, c.X, c.E, c.n_other = up, uc, V, U, ni
    else:
        c.ptr, c.col, c.X, c.E, c.n_other = ip, ic, U, V, nu
    c.h = np.diff(c.ptr)
    c.h_eff = h_eff(c.h, c.quirk and c.kind == 2)
    rng = np.random.default_rng(5)
    n = len(c.h)
    if c.kind == 1:  # ProjectU: omega per seam entity
        om = (0.05 + 0.95 * rng.random(n)).astype(np.float32)
        om[OMEGA_ZERO[0]::OMEGA_ZERO[1]] = 0.0
        c.entity_weight = om
    elif c.kind == 3:  # CVaR U step: the 0 / 1 dual weights
        c.entity_weight = (rng.random(n) < 0.4).astype(np.float32)
    elif c.kind in (2, 4):
        # omega per user (the other side), nu_u = omega_u / |H_u| and
        # item_reg_v = sum over the history of 1 / |H_u| (safer2.h:499-501)
        if c.kind == 2:
            om = (0.05 + 0.95 * rng.random(nu)).astype(np.float32)
        else:
            om = (rng.random(nu) < 0.4).astype(np.float32)
        om[NU_ZERO[0]::NU_ZERO[1]] = 0.0
        hu = np.diff(up).astype(np.float32)
        c.gram_weights = om
        c.other_weight = np.where(hu > 0, om / np.maximum(hu, 1), 0).astype(np.float32)
        inv = np.where(hu > 0, 1.0 / np.maximum(hu, 1).astype(np.float64), 0.0)
        c.entity_reg = np.bincount(np.repeat(np.arange(ni), c.h), weights=inv[ic],
                                   minlength=ni).astype(np.float32)
    return c


def reference(c):
    """The float64 half-step of case c (numpy_ref drivers), computed once."""
    k = (c.fixture, c.key, c.dim)
    if k not in _refs:
        if c.kind == 0:
            r = R.ials_side(c.ptr, c.col, c.X, c.E, c.reg, c.w, c.reg_exp)
        elif c.kind == 1:
            r = R.project_u_side(c.ptr, c.col, c.X, c.E, c.reg, c.w, c.entity_weight)
        elif c.kind == 2:
            r = R.project_v_side(c.ptr, c.col, c.X, c.E, c.reg, c.w, c.alpha, c.entity_reg,
                                 c.other_weight, c.gram_weights, c.quirk)
        elif c.kind == 3:
            r = R.cvar_u_side(c.ptr, c.col, c.X, c.E, c.reg, c.w, c.eta, c.entity_weight)
        else:
            r = R.cvar_v_side(c.ptr, c.col, c.X, c.E, c.reg, c.w, c.alpha, c.eta, c.entity_reg,
                              c.other_weight, c.gram_weights, c.quirk)
        r.setflags(write=False)
        _refs[k] = r
    return _refs[k]


def oracle_step(c):
    """The fp32 C oracle's half-step of case c, computed once."""
    k = (c.fixture, c.key, c.dim)
    if k not in _oracle:
        import oracle as O
        G = O.gramian(c.X, c.gram_weights)
        kw = {}
        if c.kind == 0:
            kw = dict(reg_exp=c.reg_exp)
        elif c.kind in (1, 3):
            kw = dict(entity_weight=c.entity_weight)
        else:
            kw = dict(alpha=c.alpha, quirk=int(c.quirk), entity_reg=c.entity_reg,
                      other_weight=c.other_weight)
        if c.kind >= 3:
            out, rc = O.step(c.ptr, c.col, c.X, G, c.kind, c.reg, c.w, stepsize=c.eta, E=c.E, **kw)
        else:
            out, rc = O.step(c.ptr, c.col, c.X, G, c.kind, c.reg, c.w, out=c.E.copy(), **kw)
        assert rc == 0, rc
        out.setflags(write=False)
        _oracle[k] = out
    return _oracle[k]
