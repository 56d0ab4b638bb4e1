"""Every device allocation of a context is owned by a DevBuf (csrc/device_buf.h):
what a context allocated is given back when it is destroyed, and a table
that is replaced frees the one it had.

The observable is frecsys_counter "live_device_bytes": the bytes all DevBufs
of the process hold.  A small witness context stays open; its reading before
a lifecycle that runs in other contexts must be its reading after they are
closed, exactly.  The lifecycles reach every buffer family of the context at
the smallest shape that does: d = 64 (history space, both bases, the weighted
kinds' uploads, CG, loss, stats, top-K, the ranking calls), d = 32 sharded
iALS++ in external-exchange mode (the block columns saved for pp_sync), d =
512 (the wide d-space workspaces and long-history slabs), d = 1024 (the
history-space wide bucket, and release_workspaces between two epochs).
"""
import numpy as np
import pytest

from test_parity_gpu import _v_inputs, _weights
from test_pp_gpu import _rix
from test_sharded_gpu import _allgather_rows, _allreduce_gram

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")
from frecsys_hip.data import _csr_from_pairs  # noqa: E402

REG, W = 0.003, 0.1
LIVE = "live_device_bytes"


@pytest.fixture()
def witness():
    ctx = fh.Context(8, 4, 4)
    yield ctx
    ctx.close()


def _csr(hists, n_items):
    """(up, uc, ip, ic) of user histories given as lists of item ids."""
    users = np.concatenate([np.full(len(h), u) for u, h in enumerate(hists)]).astype(np.int64)
    items = np.concatenate([np.asarray(h) for h in hists]).astype(np.int64)
    up, uc = _csr_from_pairs(users, items, len(hists))
    ip, ic = _csr_from_pairs(items, users, n_items)
    return up, uc, ip, ic


def _context(dim, up, uc, ip, ic):
    ctx = fh.Context(dim, len(up) - 1, len(ip) - 1)
    ctx.load_csr(fh.SIDE_USER, up, uc)
    ctx.load_csr(fh.SIDE_ITEM, ip, ic)
    ctx.init_embeddings(1, 0.1)
    return ctx


def _epoch(ctx):
    ctx.gramian(fh.SIDE_ITEM, fetch=False)
    ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, REG, W)
    ctx.gramian(fh.SIDE_USER, fetch=False)
    ctx.solve_side(fh.SIDE_ITEM, fh.KIND_IALS, REG, W)


def test_d64_lifecycle_frees_everything(witness, quirk_data):
    nu, ni, up, uc, ip, ic = quirk_data
    b0 = witness.counter(LIVE)
    ctx = _context(64, up, uc, ip, ic)
    n_eval = 40  # fold-in rows: the first users' histories
    ctx.load_csr(fh.SIDE_EVAL, up[:n_eval + 1], uc[:up[n_eval]])
    ctx.snapshot(fh.SIDE_USER)
    ctx.snapshot(fh.SIDE_ITEM)
    # iALS, Cholesky basis (l2_reg_exp = 0), then the tridiagonal one
    ctx.gramian(fh.SIDE_ITEM)
    ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, REG, W, reg_exp=0.0)
    assert ctx.work("basis_chol")[3] >= 1 and ctx.work("solve_user.hspace")[2] > 0
    ctx.gramian(fh.SIDE_USER)
    ctx.solve_side(fh.SIDE_ITEM, fh.KIND_IALS, REG, W)
    assert ctx.work("basis_tridiag")[3] >= 1
    # the weighted kinds: three uploads through their pinned staging
    om = _weights(nu)
    nu_w, item_reg = _v_inputs(nu, ni, up, ip, ic, om)
    ctx.gramian(fh.SIDE_ITEM)
    ctx.solve_side(fh.SIDE_USER, fh.KIND_WEIGHTED_U, 0.004, 0.004, entity_weight=om)
    ctx.gramian(fh.SIDE_USER, weights=om)
    ctx.solve_side(fh.SIDE_ITEM, fh.KIND_WEIGHTED_V, 0.004, 0.004, alpha=0.3,
                   entity_reg=item_reg, other_weight=nu_w)
    ctx.gramian(fh.SIDE_ITEM)
    ctx.solve_side_cg(fh.SIDE_USER, fh.KIND_IALS, REG, W)
    ctx.solve_side(fh.SIDE_EVAL, fh.KIND_IALS, REG, W)
    ctx.user_loss(fh.SIDE_USER, W, False)
    ctx.train_stats()
    assert ctx.eval_topk(10).shape == (n_eval, 10)
    ctx.recommend(fh.SIDE_USER, 10)
    rows = np.arange(30)
    cand_ptr = np.arange(0, 31 * 20, 20)
    cand = np.random.default_rng(0).integers(0, ni, cand_ptr[-1])
    ctx.rank_candidates(fh.SIDE_USER, 5, cand_ptr, cand, rows=rows)
    ctx.score_pairs(fh.SIDE_USER, rows, cand[:30])
    assert ctx.counter("hspace_reruns") == 0
    assert witness.counter(LIVE) > b0
    ctx.close()
    assert witness.counter(LIVE) == b0


def test_sharded_pp_step_frees_block_columns(witness, quirk_data):
    """External-exchange iALS++ at world 2: pp_step saves the block columns
    of every row for pp_sync."""
    nu, ni, up, uc, ip, ic = quirk_data
    dim = 32
    b0 = witness.counter(LIVE)
    urix, irix = _rix(uc)
    ctxs = []
    for r in range(2):
        c = fh.Context(dim, nu, ni, device=0)
        c.comm_init(2, r, None)
        c.load_csr(fh.SIDE_USER, up, uc)
        c.load_csr(fh.SIDE_ITEM, ip, ic)
        c.init_embeddings(1, 0.1)
        c.pp_set_rating_index(fh.SIDE_USER, urix)
        c.pp_set_rating_index(fh.SIDE_ITEM, irix)
        c.pp_predict(fh.SIDE_USER)
        ctxs.append(c)
    _allreduce_gram(ctxs, fh.SIDE_ITEM)
    before = witness.counter(LIVE)
    for c in ctxs:
        c.pp_step(fh.SIDE_USER, 0, dim, REG, W)
    # the saved columns ([n][bw] floats) of both ranks are among what the step allocated
    assert witness.counter(LIVE) - before >= 2 * nu * dim * 4
    _allgather_rows(ctxs, fh.SIDE_USER)
    for c in ctxs:
        c.pp_sync(fh.SIDE_USER)
    for c in ctxs:
        c.close()
    assert witness.counter(LIVE) == b0


def test_d512_wide_workspaces_freed(witness):
    """d = 512: the item every user has (more than twice the slab rows of the
    wide SYRK) is solved in d-space through the batch workspace, the
    pre-split table and the long-history slabs."""
    rng = np.random.default_rng(3)
    n_users, n_items = 4200, 40
    hists = [[0] + list(1 + rng.choice(n_items - 1, 3, replace=False)) for _ in range(n_users)]
    up, uc, ip, ic = _csr(hists, n_items)
    b0 = witness.counter(LIVE)
    ctx = _context(512, up, uc, ip, ic)
    ctx.gramian(fh.SIDE_USER, fetch=False)
    ctx.solve_side(fh.SIDE_ITEM, fh.KIND_IALS, REG, W)
    assert ctx.work("solve_item.dspace")[2] > 0
    held = witness.counter(LIVE)
    ctx.release_workspaces()
    assert witness.counter(LIVE) < held
    ctx.solve_side(fh.SIDE_ITEM, fh.KIND_IALS, REG, W)  # sized again
    assert witness.counter(LIVE) == held
    ctx.close()
    assert witness.counter(LIVE) == b0


def test_d1024_release_workspaces_bitwise(witness):
    """d = 1024: one user in the history-space wide bucket (256 < h <= 512).
    Releasing the workspaces between two epochs lowers the counter and
    changes no bit of the second epoch."""
    rng = np.random.default_rng(4)
    n_users, n_items = 24, 320
    hists = [rng.choice(n_items, 300 if u == 0 else int(rng.integers(5, 20)), replace=False)
             for u in range(n_users)]
    data = _csr(hists, n_items)
    b0 = witness.counter(LIVE)

    def two_epochs(release):
        ctx = _context(1024, *data)
        _epoch(ctx)
        assert ctx.work("solve_user.hspace")[2] == n_users
        if release:
            held = witness.counter(LIVE)
            ctx.release_workspaces()
            assert witness.counter(LIVE) < held
        _epoch(ctx)
        assert ctx.counter("hspace_reruns") == 0
        out = ctx.get_embeddings(fh.SIDE_USER), ctx.get_embeddings(fh.SIDE_ITEM)
        ctx.close()
        return out

    U0, V0 = two_epochs(False)
    assert witness.counter(LIVE) == b0
    U1, V1 = two_epochs(True)
    assert witness.counter(LIVE) == b0
    np.testing.assert_array_equal(U1, U0)
    np.testing.assert_array_equal(V1, V0)


def test_replaced_tables_free_the_old(witness, quirk_data):
    """A CSR loaded twice and a snapshot taken twice hold what they held after
    the first time."""
    nu, ni, up, uc, ip, ic = quirk_data
    b0 = witness.counter(LIVE)
    ctx = fh.Context(64, nu, ni)

    def load():
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.load_csr(fh.SIDE_ITEM, ip, ic)
        ctx.load_csr(fh.SIDE_EVAL, up[:41], uc[:up[40]])
        ctx.snapshot(fh.SIDE_USER)
        ctx.snapshot(fh.SIDE_ITEM)
        return witness.counter(LIVE)

    first = load()
    assert first > b0
    assert load() == first
    ctx.close()
    assert witness.counter(LIVE) == b0
