"""Model.explain / Model.explain_fold_in (frecsys_model_explain*) on trained
models: conftest.make_quirk_data() (700 x 400), dims 20 and 64, two epochs.

ials, safer2, erm_mf, cvar_mf: explain_fold_in's scores are the scores
recommend_fold_in lists for the same histories and items, within twice
TOL_ROW ||v_t|| ||x|| (both sides carry rounding; x from the float64 reference on
the fetched tables); the contributions sum to the score; explain(users) is
explain_fold_in of those users' training histories bit for bit.
ialspp, safer2pp: contributions and scores against tests/explain_ref.py on the
fetched tables (the exact minimiser of the objective their block steps
descend); nothing is asserted against their 8-epoch fold-in.
A model loaded serve-only answers explain_fold_in with the saving model's
bytes and refuses explain(users).
"""
import numpy as np
import pytest

import cg_ref as C
import explain_ref as X
import frecsys_hip as fh
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

TOL_ROW = X.TOL_ROW
IDLE_USER = 5
TOP, NT = 10, 10


@pytest.fixture(scope="module")
def data():
    nu, ni, up, uc, ip, ic = make_quirk_data()
    users = np.repeat(np.arange(nu, dtype=np.int32), np.diff(up))
    items = np.asarray(uc, dtype=np.int32)
    lens = np.diff(up)
    order = np.argsort(lens, kind="stable")
    pick = [IDLE_USER] + [int(u) for u in order[np.linspace(1, nu - 1, 11).astype(int)]]
    assert lens[IDLE_USER] == 0 and lens[pick[-1]] >= 300 and lens[pick[1]] <= 5
    q = np.array(pick, dtype=np.int64)
    hp = np.concatenate([[0], np.cumsum(lens[q])]).astype(np.int64)
    hi = np.concatenate([uc[up[u]:up[u + 1]] for u in q]).astype(np.int32)
    return dict(nu=nu, ni=ni, users=users, items=items, q=q, hp=hp, hi=hi)


def _flags(name, dim):
    f = dict(dim=dim, seed=1, print_train_stats=False, stdev=0.1)
    if name in ("ials", "ialspp"):
        f.update(l2_reg=0.003, uobs_weight=0.1)
    else:
        f.update(l2_reg=0.004, uobs_weight=0.004, bandwidth=0.15, alpha=0.3)
    if name in ("ialspp", "safer2pp"):
        f.update(block_size=max(8, dim // 2))
    return f


class ModelCase:
    """What explain_ref needs of a trained model: the item table and the solve
    parameters of the model's fold-in (omega = 1)."""

    def __init__(self, name, dim, V, n_rows):
        f = _flags(name, dim)
        self.kind = C.KIND_IALS if name in ("ials", "ialspp") else C.KIND_U
        self.dim, self.X, self.n_other = dim, V, V.shape[0]
        self.reg, self.w, self.reg_exp, self.alpha = f["l2_reg"], f["uobs_weight"], 1.0, 0.3
        self.omega = np.ones(n_rows, np.float32)
        self.gram_weights = None

    lam = C.Case.lam


def _trained(name, dim, d):
    m = fh.Model(name, d["users"], d["items"], **_flags(name, dim))
    m.initialize()
    m.train(2)
    return m


def _reference(name, dim, m, d, tp, tgt):
    V = m.context().get_embeddings(fh.SIDE_ITEM)
    mc = ModelCase(name, dim, V, len(d["q"]))
    G = C.gram(mc, np.float64)
    return mc, [X.explain_entity(mc, e, d["hi"][d["hp"][e]:d["hp"][e + 1]], tgt[tp[e]:tp[e + 1]], G)
                for e in range(len(d["q"]))]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _sums_to_score(score, full, fp):
    """A float32 sum of h terms in any order is within (h - 1) 2^-24 sum |c_j|
    of the exact sum (twice that allowed)."""
    for p in range(len(score)):
        c = full[fp[p]:fp[p + 1]].astype(np.float64)
        assert abs(c.sum() - float(score[p])) <= len(c) * 2.0 ** -23 * np.abs(c).sum()


@pytest.mark.parametrize("dim", [20, 64])
@pytest.mark.parametrize("name", ["ials", "safer2", "erm_mf", "cvar_mf"])
def test_explains_the_fold_in_scores(name, dim, data):
    d = data
    m = _trained(name, dim, d)
    n = len(d["q"])
    rec_items, rec_scores = m.recommend_fold_in(d["hp"], d["hi"], NT, exclude_seen=False)
    assert (rec_items >= 0).all()
    tp = (np.arange(n + 1) * NT).astype(np.int64)
    tgt = rec_items.reshape(-1).astype(np.int32)
    score, items, vals, full, fp = m.explain_fold_in(d["hp"], d["hi"], tp, tgt, top=TOP, full=True)
    mc, ref = _reference(name, dim, m, d, tp, tgt)
    worst = 0.0
    for e in range(n):
        x = ref[e][2]
        for t in range(NT):
            p = e * NT + t
            if d["hp"][e + 1] == d["hp"][e]:
                assert score[p] == 0.0 and rec_scores[e, t] == 0.0
                assert (items[p] == -1).all() and not vals[p].any()
                continue
            bound = np.linalg.norm(mc.X[tgt[p]].astype(np.float64)) * np.linalg.norm(x)
            worst = max(worst, abs(float(score[p]) - float(rec_scores[e, t])) / bound)
    print(f"{name} d{dim}: worst |explain - fold-in score| / (|v| |x|) {worst:.2e}")
    assert worst <= 2 * TOL_ROW
    _sums_to_score(score, full, fp)
    _same(m.explain(d["q"], tp, tgt, top=TOP, full=True), (score, items, vals, full, fp))
    m.close()


@pytest.mark.parametrize("dim", [20, 64])
@pytest.mark.parametrize("name", ["ialspp", "safer2pp"])
def test_block_models_explain_the_exact_minimiser(name, dim, data):
    d = data
    m = _trained(name, dim, d)
    n = len(d["q"])
    tp = (np.arange(n + 1) * NT).astype(np.int64)
    tgt = np.random.default_rng(dim).integers(0, d["ni"], n * NT).astype(np.int32)
    score, items, vals, full, fp = m.explain_fold_in(d["hp"], d["hi"], tp, tgt, top=TOP, full=True)
    mc, ref = _reference(name, dim, m, d, tp, tgt)
    worst_c = worst_s = 0.0
    for e in range(n):
        contrib, sref, x = ref[e]
        for t in range(NT):
            p = e * NT + t
            got = full[fp[p]:fp[p + 1]].astype(np.float64)
            if len(got) == 0:
                assert score[p] == 0.0
                continue
            worst_c = max(worst_c, np.linalg.norm(got - contrib[:, t]) / np.linalg.norm(contrib[:, t]))
            bound = np.linalg.norm(mc.X[tgt[p]].astype(np.float64)) * np.linalg.norm(x)
            worst_s = max(worst_s, abs(float(score[p]) - sref[t]) / bound)
    print(f"{name} d{dim}: worst pair rel err {worst_c:.2e}, score {worst_s:.2e}")
    assert worst_c < TOL_ROW and worst_s <= TOL_ROW
    _sums_to_score(score, full, fp)
    _same(m.explain(d["q"], tp, tgt, top=TOP, full=True), (score, items, vals, full, fp))
    m.close()


def test_serve_only_model(data, tmp_path):
    d = data
    a = _trained("ials", 20, d)
    n = len(d["q"])
    tp = (np.arange(n + 1) * NT).astype(np.int64)
    tgt = np.random.default_rng(1).integers(0, d["ni"], n * NT).astype(np.int32)
    want = a.explain_fold_in(d["hp"], d["hi"], tp, tgt, top=TOP, full=True)
    path = str(tmp_path / "serve.frecsys")
    a.save(path, include_data=False)
    a.close()
    b = fh.Model.load(path)
    _same(b.explain_fold_in(d["hp"], d["hi"], tp, tgt, top=TOP, full=True), want)
    for full in (False, True):
        with pytest.raises(fh.FrecsysError) as e:
            b.explain(d["q"], tp, tgt, top=TOP, full=full)
        assert e.value.code == fh.ERR_INVALID
    b.close()
