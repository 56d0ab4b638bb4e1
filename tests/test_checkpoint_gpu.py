"""Model checkpoints on the GPU: a resumed run is the uninterrupted run bit for
bit, a loaded model serves the saved model's bits, the file is what DESIGN.md
3.16 says (read back by tests/checkpoint_ref.py, which never imports the
library), serve-only and warm-start loads, refusals, atomic save.

Data: conftest.make_quirk_data() as tuples (700 x 400: an idle user 5 and an
idle item 9 whose rows keep their seeded init, every history-space bucket, the
tail-quirk lengths).  Dims 16 (small-kernel path), 64 (history space and
d-space) and, for iALS, 300 (padded to 512: the wide path's derived tables are
rebuilt from a load).  Every comparison is an equality of bytes."""
import os

import numpy as np
import pytest

import checkpoint_ref as R
import frecsys_hip as fh
from conftest import make_quirk_data

pytestmark = pytest.mark.gpu

IDLE_USER, IDLE_ITEM = 5, 9
DUAL = ("safer2", "safer2pp", "erm_mf", "cvar_mf")


@pytest.fixture(scope="module")
def data():
    nu, ni, up, uc, ip, ic = make_quirk_data()
    users = np.repeat(np.arange(nu, dtype=np.int32), np.diff(up))
    items = np.asarray(uc, dtype=np.int32)
    assert up[IDLE_USER + 1] == up[IDLE_USER] and ip[IDLE_ITEM + 1] == ip[IDLE_ITEM]
    return nu, ni, users, items, up, uc


def _flags(name, dim, **more):
    f = dict(dim=dim, seed=1, print_train_stats=False, stdev=0.1)
    if name in ("ials", "ialspp"):
        f.update(l2_reg=0.003, uobs_weight=0.1)
    else:
        f.update(l2_reg=0.004, uobs_weight=0.004, bandwidth=0.15, alpha=0.3)
    if name in ("ialspp", "safer2pp"):
        f.update(block_size=max(8, dim // 2))  # two column blocks
    f.update(more)
    return f


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _state(m):
    """Everything a run is compared by, as named byte strings."""
    ctx = m.context()
    out = {"U": ctx.get_embeddings(fh.SIDE_USER), "V": ctx.get_embeddings(fh.SIDE_ITEM),
           "epochs": np.int64(m.epochs)}
    try:
        w, l, r, xi = m.dual_state()
        out.update(omega=w, loss=l, item_reg=r, xi=np.float32(xi))
    except fh.FrecsysError as e:  # iALS / iALS++ have no dual weights
        assert e.code == fh.ERR_INVALID
    return out


def _assert_same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert _same(a[k], b[k]), f"{what}: {k} differs"


CASES = [(n, d, {}) for n in ("ials", "ialspp", "safer2", "safer2pp", "erm_mf", "cvar_mf")
         for d in (16, 64)]
CASES += [("safer2", 16, {"use_snr": True}), ("safer2", 64, {"use_snr": True}),
          ("safer2pp", 16, {"use_snr": True}), ("ials", 300, {})]


@pytest.mark.parametrize("name,dim,more", CASES,
                         ids=[f"{n}-d{d}" + ("-snr" if m else "") for n, d, m in CASES])
def test_resume_is_the_uninterrupted_run(tmp_path, data, name, dim, more):
    """train(3) against train(2), save, close, load, train(1): U, V, omega,
    the user losses, item_reg, xi and epochs equal bitwise -- with the tuples
    read from the file and with the tuples passed by the caller."""
    nu, ni, users, items, _, _ = data
    f = _flags(name, dim, **more)
    a = fh.Model(name, users, items, **f)
    a.initialize()
    a.train(3)
    want = _state(a)
    a.close()
    assert want["epochs"] == 3

    b = fh.Model(name, users, items, **f)
    b.initialize()
    b.train(2)
    path = str(tmp_path / "b.frecsys")
    b.save(path)
    mid = _state(b)
    b.close()
    info = fh.model_file_info(path)
    assert info["epochs_trained"] == 2 and info["has_data"] and info["model_name"] == name

    for how, args in (("tuples from the file", {}),
                      ("tuples from the caller", dict(users=users, items=items))):
        c = fh.Model.load(path, **args)
        assert (c.n_users, c.n_items, c.dim, c.epochs) == (nu, ni, dim, 2)
        _assert_same_state(_state(c), mid, how + ", before training")
        c.initialize()  # a no-op on a loaded model
        _assert_same_state(_state(c), mid, how + ", after initialize()")
        c.train(1)
        _assert_same_state(_state(c), want, how)
        c.close()


def _queries(data):
    nu, ni, users, items, up, uc = data
    rows = np.array([0, 1, 2, 3, IDLE_USER, 6, 7, 8, 100, 355, 699], dtype=np.int64)
    rng = np.random.default_rng(5)
    # ground truth: 3 random items per row; fold-in histories: the rows' own
    gt_ptr = np.arange(len(rows) + 1, dtype=np.int64) * 3
    gt_items = np.concatenate([rng.choice(ni, 3, replace=False) for _ in rows]).astype(np.int32)
    hist_rows = rows[rows != IDLE_USER]
    hp = np.concatenate([[0], np.cumsum(np.diff(up)[hist_rows])]).astype(np.int64)
    hi = np.concatenate([uc[up[r]:up[r + 1]] for r in hist_rows]).astype(np.int32)
    return rows, gt_ptr, gt_items, hp, hi, len(hist_rows)


def _serve(m, data, exclude_seen_too=True):
    rows, gt_ptr, gt_items, hp, hi, nh = _queries(data)
    out = {}
    for ex in ((True, False) if exclude_seen_too else (False,)):
        out[f"rec{ex}"] = m.recommend(rows, 10, exclude_seen=ex)
    out["fold"] = m.recommend_fold_in(hp, hi, 10)
    out["sim"] = m.similar_items(np.array([0, 3, IDLE_ITEM, 57, 399]), 10)
    pu = np.repeat(rows, 4)
    pi = np.tile(np.array([0, IDLE_ITEM, 200, 399], dtype=np.int32), len(rows))
    out["score"] = (m.score(pu, pi),)
    if exclude_seen_too:
        er = m.evaluate_ranks(rows, gt_ptr, gt_items)
        out["ranks"] = (er["rank"], er["eligible"], er["mrr"], er["auc"], er["mrr_cvar"],
                        er["auc_cvar"], np.float32(er["mean_mrr"]), np.float32(er["mean_auc"]))
    ef = m.evaluate_fold_in(hp, hi, gt_ptr[:nh + 1], gt_items[:3 * nh])
    out["eval_fold"] = (ef["recall"], ef["ndcg"], ef["mean_recall"], ef["mean_ndcg"],
                        ef["recall_cvar"], ef["ndcg_cvar"])
    return out


def _assert_same_answers(a, b):
    assert a.keys() == b.keys()
    for k in a:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert _same(x, y), f"{k}[{i}] differs"


@pytest.mark.parametrize("name,dim", [("ials", 64), ("safer2", 16), ("ials", 300)])
def test_loaded_model_serves_the_same_bits(tmp_path, data, name, dim):
    """No train() on the loaded model: recommend with and without exclude_seen,
    recommend_fold_in, similar_items, score, evaluate_ranks, evaluate_fold_in
    on rows that include the idle user."""
    _, _, users, items, _, _ = data
    a = fh.Model(name, users, items, **_flags(name, dim))
    a.initialize()
    a.train(2)
    path = str(tmp_path / "a.frecsys")
    a.save(path)
    want = _serve(a, data)
    a.close()
    b = fh.Model.load(path)
    _assert_same_answers(_serve(b, data), want)
    b.close()


@pytest.mark.parametrize("name", ["ials", "safer2"])
def test_file_is_what_the_specification_says(tmp_path, data, name):
    nu, ni, users, items, _, _ = data
    f = _flags(name, 16, use_snr=(name == "safer2"))
    m = fh.Model(name, users, items, **f)
    ctx = m.context()
    idle_u = ctx.get_embeddings(fh.SIDE_USER)[IDLE_USER].copy()
    idle_v = ctx.get_embeddings(fh.SIDE_ITEM)[IDLE_ITEM].copy()
    m.initialize()
    m.train(2)
    path = str(tmp_path / "m.frecsys")
    m.save(path)
    got = R.read(path)  # asserts the layout rules and every checksum in numpy
    assert _same(got["U"], ctx.get_embeddings(fh.SIDE_USER))
    assert _same(got["V"], ctx.get_embeddings(fh.SIDE_ITEM))
    assert _same(got["users"], users) and _same(got["items"], items)
    assert got["flags"] == 1
    cfg = got["config"]
    assert cfg["model_name"] == name and cfg["epochs_trained"] == 2
    assert (cfg["n_users"], cfg["n_items"], cfg["n_tuples"]) == (nu, ni, len(users))
    defaults = dict(R.CONFIG_DEFAULTS, **{k: v for k, v in f.items()})
    for field, is_float in R.CONFIG_FIELDS:
        want = defaults[field]
        if is_float:
            assert np.float32(cfg[field]) == np.float32(want), field
        else:
            assert cfg[field] == int(want), field
    # the idle rows keep their seeded init: non-zero, as before training
    assert got["U"][IDLE_USER].any() and _same(got["U"][IDLE_USER], idle_u)
    assert got["V"][IDLE_ITEM].any() and _same(got["V"][IDLE_ITEM], idle_v)
    if name == "safer2":
        w, l, r, xi = m.dual_state()
        assert _same(got["omega"], w) and _same(got["loss"], l) and _same(got["item_reg"], r)
        assert int(got["state"]["xi_bits"]) == int(np.float32(xi).view(np.uint32))
        assert len(got["state"]["snr_rng"].split()) == 625
        assert "snr_pending" not in got["state"]
    else:
        assert got["state"] == {} and "OMEGA" not in got["raw"]
    # without the tuples: the same file minus USERS / ITEMS, same tuples_checksum
    m.save(path + ".nodata", include_data=False)
    bare = R.read(path + ".nodata")
    assert bare["flags"] == 0 and "users" not in bare
    assert bare["config"] == cfg and _same(bare["U"], got["U"]) and _same(bare["V"], got["V"])
    assert cfg["tuples_checksum"] == R.tuples_checksum(users, items)
    m.close()


@pytest.mark.parametrize("name", ["ials", "safer2"])
def test_serve_only(tmp_path, data, name):
    _, _, users, items, _, _ = data
    a = fh.Model(name, users, items, **_flags(name, 16))
    a.initialize()
    a.train(2)
    path = str(tmp_path / "serve.frecsys")
    a.save(path, include_data=False)
    want = _serve(a, data, exclude_seen_too=False)
    a.close()
    b = fh.Model.load(path)
    assert b.epochs == 2
    _assert_same_answers(_serve(b, data, exclude_seen_too=False), want)
    rows = _queries(data)[0]
    b.initialize()  # a loaded model is initialised: a no-op
    gt_ptr, gt_items = _queries(data)[1:3]
    for call in (lambda: b.train(1), lambda: b.recommend(rows, 10, exclude_seen=True),
                 lambda: b.evaluate_ranks(rows, gt_ptr, gt_items, exclude_seen=True)):
        with pytest.raises(fh.FrecsysError) as e:
            call()
        assert e.value.code == fh.ERR_INVALID and "serve-only" in str(e.value)
    # the model stays usable, and can be saved again with what it knows
    _assert_same_answers(_serve(b, data, exclude_seen_too=False), want)
    b.save(path + ".again")
    assert R.read(path + ".again")["raw"] == R.read(path)["raw"]
    b.close()


def test_warm_start_into_a_grown_id_space(tmp_path, data):
    nu, ni, users, items, _, _ = data
    f = _flags("safer2", 16)
    a = fh.Model("safer2", users, items, **f)
    a.initialize()
    a.train(2)
    path = str(tmp_path / "a.frecsys")
    a.save(path)
    a.close()
    stored = R.read(path)
    u2 = np.concatenate([users, [nu, nu + 1, nu + 2, 0]]).astype(np.int32)
    i2 = np.concatenate([items, [0, ni, ni + 1, ni + 1]]).astype(np.int32)
    fresh = fh.Model("safer2", u2, i2, **f)
    fctx = fresh.context()
    U0, V0 = fctx.get_embeddings(fh.SIDE_USER), fctx.get_embeddings(fh.SIDE_ITEM)
    fresh.close()
    b = fh.Model.load(path, users=u2, items=i2, tables_only=True)
    assert (b.n_users, b.n_items, b.dim, b.epochs) == (nu + 3, ni + 2, 16, 0)
    ctx = b.context()
    U, V = ctx.get_embeddings(fh.SIDE_USER), ctx.get_embeddings(fh.SIDE_ITEM)
    assert _same(U[:nu], stored["U"]) and _same(V[:ni], stored["V"])
    assert _same(U[nu:], U0[nu:]) and _same(V[ni:], V0[ni:])
    w, l, r, xi = b.dual_state()  # a new model's: nothing restored
    assert (w == np.float32(0.3)).all() and not l.any() and not r.any() and xi == 0.0
    b.initialize()
    b.train(1)
    U, V = ctx.get_embeddings(fh.SIDE_USER), ctx.get_embeddings(fh.SIDE_ITEM)
    assert np.isfinite(U).all() and np.isfinite(V).all() and b.epochs == 1
    b.close()


def test_refusals(tmp_path, data):
    nu, ni, users, items, _, _ = data
    a = fh.Model("ials", users, items, **_flags("ials", 16))
    a.train(1)
    path = str(tmp_path / "a.frecsys")
    a.save(path)
    a.save(path + ".nodata", include_data=False)
    a.close()
    changed = items.copy()
    changed[17] = (changed[17] + 1) % ni
    swapped = np.arange(len(users))
    swapped[[3, 4]] = [4, 3]
    keep = users < nu - 1  # one user fewer
    cases = {
        "one tuple changed": dict(users=users, items=changed),
        "another order": dict(users=users[swapped], items=items[swapped]),
        "fewer tuples": dict(users=users[:-1], items=items[:-1]),
        "dim overridden": dict(dim=32),
        "model_name overridden": dict(model_name="ialspp"),
        "parity_quirks overridden": dict(parity_quirks=0),
        "tables_only, smaller id space": dict(users=users[keep], items=items[keep], tables_only=True),
        "tables_only without tuples": dict(tables_only=True),
    }
    for p in (path, path + ".nodata"):
        for what, args in cases.items():
            with pytest.raises(fh.FrecsysError) as e:
                fh.Model.load(p, **args)
            assert e.value.code == fh.ERR_INVALID, (what, str(e.value))
    for what in ("one tuple changed", "another order"):
        with pytest.raises(fh.FrecsysError) as e:
            fh.Model.load(path, **cases[what])
        assert "tuples_checksum" in str(e.value)
    # the right tuples are accepted by both files
    for p in (path, path + ".nodata"):
        m = fh.Model.load(p, users=users, items=items)
        assert m.epochs == 1
        m.close()


def test_save_is_atomic(tmp_path, data):
    _, _, users, items, _, _ = data
    m = fh.Model("ials", users, items, **_flags("ials", 16))
    m.train(1)
    first, other = str(tmp_path / "first.frecsys"), str(tmp_path / "other.frecsys")
    m.save(first)
    m.save(other)
    one = R.read(first)
    m.train(1)
    m.save(first)  # over an existing checkpoint
    two = R.read(first)
    assert two["config"]["epochs_trained"] == 2 and not _same(two["U"], one["U"])
    with pytest.raises(fh.FrecsysError) as e:
        m.save(str(tmp_path / "no_such_dir" / "m.frecsys"))
    assert e.value.code == fh.ERR_IO == 8
    assert sorted(os.listdir(tmp_path)) == ["first.frecsys", "other.frecsys"]
    ctx = m.context()
    for p, epochs, ref in ((first, 2, two), (other, 1, one)):
        b = fh.Model.load(p)
        assert b.epochs == epochs
        assert _same(b.context().get_embeddings(fh.SIDE_USER), ref["U"])
        b.close()
    assert _same(ctx.get_embeddings(fh.SIDE_USER), two["U"])
    m.close()
