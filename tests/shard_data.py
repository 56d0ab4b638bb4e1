"""The shard seams of the sharded (N-rank) path: fixtures, their expected
shard bounds, the properties under which test_shard_seam_gpu.py means
anything, and the exchange helpers a test performs between the ranks.

Ranks are W contexts of one process on device 0 in external-exchange mode
(comm_init(W, r, None)), as in test_sharded_gpu.py.  Two fixtures, both over
the 704 rows of seam_data's other side and in both orientations:

  seam  seam_data unchanged (104 entities, 19,215 nnz).  Its histories grow
        with the index, so an nnz-balanced split cuts it into shards that lie
        wholly in history space, wholly in d-space, in one bucket, or hold
        two or three entities (447 | 448, 383..385, 415..417).
  skew  10 entities with h = 0, 3, 640, 1, 0, 2, 33, 600, 0, 0, drawn like
        seam_data's histories.  One entity holds more than two shares of the
        nnz, so partition_rows yields bounds[r] == bounds[r + 1] (an empty
        shard), and the idle entities behind the last heavy one make a shard
        whose queue is not empty but holds no work.

partition() restates capi.hip partition_rows; BOUNDS are its results on the
two fixtures, written out (test_shard_seam_cpu.py holds the restatement, the
C function and the constants to each other).

The weights (omega, nu, item_reg) of a skew case are seam_data.build_case's;
its float64 reference is seam_data.reference, its fp32 oracle step
seam_data.oracle_step -- no (kind, dim) pair is left out of the skew cases:
the oracle stays below a quarter of the row bar on all of them
(test_shard_seam_cpu.py).

Row subsets: the rotation of the other side covers only the
rows a shard's history-space entities read when those are at most 70 % of
the table.  At W = 8 and W = 16 the seam fixture has shards on either side of
that (subset_rows); variant() redraws the histories of one shard from a band
of the other side's rows, so one context can be taken from the plain pass to
a subset and from one subset to another.
"""
import bisect
import types

import numpy as np

import seam_data as S

N_OTHER = S.N_OTHER
SKEW_H = (0, 3, 640, 1, 0, 2, 33, 600, 0, 0)
SKEW_SEED = 37
SUBSET_MAX = 0.7           # hspace_rows: a list when it is at most this share of the table
HSPACE_MAX_H = {"narrow": 224, "wide": 256}  # Dp 64..256 | the wide dims' buckets

# fixture, world: the bounds of partition_rows on the solved side
BOUNDS = {
    ("seam", 3): (0, 37, 51, 104),
    ("seam", 8): (0, 23, 32, 39, 44, 49, 59, 81, 104),
    ("seam", 16): (0, 17, 23, 28, 32, 36, 39, 42, 44, 47, 49, 52, 59, 71, 81, 91, 104),
    ("skew", 2): (0, 3, 10),
    ("skew", 3): (0, 3, 8, 10),
    ("skew", 4): (0, 3, 3, 8, 10),
    ("skew", 8): (0, 3, 3, 3, 3, 8, 8, 8, 10),
}
WORLDS = {"seam": (3, 8, 16), "skew": (2, 3, 4, 8)}


def partition(row_ptr, parts):
    """capi.hip partition_rows: rank r starts at the first row whose nnz prefix
    reaches r * nnz / parts (lower_bound), never before the rank below it."""
    rp = [int(x) for x in row_ptr]
    n = len(rp) - 1
    nnz = rp[n] - rp[0]
    b = [0]
    for r in range(1, parts):
        x = bisect.bisect_left(rp, rp[0] + (nnz * r) // parts)
        b.append(min(max(x, b[-1]), n))
    b.append(n)
    return b


def make_skew_data(seed=SKEW_SEED):
    """The skew fixture in make_seam_data's form (hists, labels, n_other)."""
    rng = np.random.default_rng(seed)
    hists = [np.asarray(rng.permutation(N_OTHER)[:h], np.int64) for h in SKEW_H]
    labels = [f"skew{h}" if h else "idle" for h in SKEW_H]
    return types.SimpleNamespace(hists=hists, labels=labels, n_other=N_OTHER)


def variant(sd, lo, hi, row_lo, row_hi, seed):
    """sd with the histories of entities [lo, hi) replaced by fresh draws of
    the same lengths from the other side's rows [row_lo, row_hi)."""
    rng = np.random.default_rng(seed)
    hists = list(sd.hists)
    for e in range(lo, hi):
        h = len(hists[e])
        assert h <= row_hi - row_lo
        hists[e] = np.asarray(row_lo + rng.permutation(row_hi - row_lo)[:h], np.int64)
    return types.SimpleNamespace(hists=hists, labels=sd.labels, n_other=sd.n_other)


_data, _cases = {}, {}


def fixture_data(fixture):
    """{"sd", "user": as_users(sd), "item": as_items(sd)} of a fixture:
    "seam", "skew", or a variant of the seam fixture registered by
    register_variant."""
    if fixture not in _data:
        if fixture == "seam":
            sd = S.seam_data()
        elif fixture == "skew":
            sd = make_skew_data()
        else:
            raise KeyError(fixture)
        _data[fixture] = dict(sd=sd, user=S.as_users(sd), item=S.as_items(sd))
    return _data[fixture]


def register_variant(name, lo, hi, row_lo, row_hi, seed):
    if name not in _data:
        sd = variant(S.seam_data(), lo, hi, row_lo, row_hi, seed)
        _data[name] = dict(sd=sd, user=S.as_users(sd), item=S.as_items(sd))
    return _data[name]


def case(fixture, key, dim):
    """seam_data.seam_case for any fixture (the seam fixture's are the same
    objects, so its references are shared with test_seam_gpu.py)."""
    if fixture == "seam":
        return S.seam_case(key, dim)
    if (fixture, key, dim) not in _cases:
        d = fixture_data(fixture)
        _cases[fixture, key, dim] = S.build_case(key, dim, d["sd"].labels,
                                                 d[S.KINDS[key]["seam"]], fixture)
    return _cases[fixture, key, dim]


def pp_case(fixture, key, dim):
    """pp_ref.pp_case for any fixture: the case plus the rating indices (the
    file position of every CSR entry, from the fixture's own pair list)."""
    c = case(fixture, key, dim)
    ent, oth = S._pairs(fixture_data(fixture)["sd"])
    users_file, items_file = (ent, oth) if c.seam == "user" else (oth, ent)
    urix = np.argsort(users_file, kind="stable").astype(np.int32)
    irix = np.argsort(items_file, kind="stable").astype(np.int32)
    np.testing.assert_array_equal(c.uc, items_file[urix])
    np.testing.assert_array_equal(c.ic, users_file[irix])
    return types.SimpleNamespace(c=c, key=key, dim=dim, urix=urix, irix=irix,
                                 rix=urix if c.seam == "user" else irix, nnz=len(c.uc),
                                 live=np.nonzero(c.h > 0)[0])


def solved_ptr(fixture):
    """Row pointer of the fixture's own entities (the same in both orientations)."""
    return fixture_data(fixture)["user"][2]


def shards(bounds):
    return list(zip(bounds[:-1], bounds[1:]))


def shard_kinds(h, h_eff, bounds, threshold):
    """One set of words per shard: "empty" (no entity), "idle" (entities, none
    with a history), "below" / "above" (every live entity at or below / above
    the history-space threshold), "straddle" (both), "small" (one to three
    entities)."""
    out = []
    for lo, hi in shards(bounds):
        he = np.asarray(h_eff[lo:hi])
        live = he[np.asarray(h[lo:hi]) > 0]
        k = set()
        if hi == lo:
            k.add("empty")
        elif len(live) == 0:
            k.add("idle")
        elif (live <= threshold).all():
            k.add("below")
        elif (live > threshold).all():
            k.add("above")
        else:
            k.add("straddle")
        if 1 <= hi - lo <= 3:
            k.add("small")
        out.append(k)
    return out


def check_coverage(found):
    """What the fixtures must provide between them (found: the union of
    shard_kinds over every fixture, world and threshold used)."""
    for k in ("empty", "idle", "below", "above", "straddle", "small"):
        assert k in found, k


def subset_rows(c, lo, hi, max_h):
    """(history-space entities of shard [lo, hi) of case c, size of the row
    list hspace_rows builds for them): the distinct rows of the other side
    they read, and row 0, which the kernels load for a tile's padding rows."""
    rows, n = set(), 0
    for e in range(lo, hi):
        if 0 < c.h_eff[e] <= max_h:
            rows.update(c.col[c.ptr[e]:c.ptr[e + 1]].tolist())
            n += 1
    if n:
        rows.add(0)
    return n, len(rows)


def takes_subset(n_rows_read, n_other=N_OTHER):
    """hspace_rows' decision: a row list unless it is most of the table."""
    return not float(n_rows_read) > SUBSET_MAX * float(n_other)


# ---- the exchange a test performs between the ranks (external-exchange mode) ----
def contexts(world, dim, nu, ni, up, uc, ip, ic):
    import frecsys_hip as fh
    ctxs = []
    for r in range(world):
        c = fh.Context(dim, nu, ni, device=0)
        if world > 1:
            c.comm_init(world, r, None)
        c.load_csr(fh.SIDE_USER, up, uc)
        c.load_csr(fh.SIDE_ITEM, ip, ic)
        c.init_embeddings(1, 0.1)
        ctxs.append(c)
    return ctxs


def allreduce_gram(ctxs, side, weights=None):
    parts = [c.gramian(side, weights) for c in ctxs]
    if len(ctxs) == 1:
        return parts[0]
    # the exchange frecsys_gramian does over RCCL: every group slab from its owner
    slabs = None
    for c in ctxs:
        ng, lo, hi, _ = c.gram_groups(side)
        mine = c.get_gram_groups(side)
        if slabs is None:
            slabs = np.zeros_like(mine)
        assert not mine[:lo].any() and not mine[hi:].any()  # only its own groups
        slabs[lo:hi] = mine[lo:hi]
    owned = sorted(c.gram_groups(side)[1:3] for c in ctxs)
    assert owned[0][0] == 0 and owned[-1][1] == slabs.shape[0]
    assert all(a[1] == b[0] for a, b in zip(owned, owned[1:]))  # the ranks tile the groups
    for c in ctxs:
        c.set_gram_groups(side, slabs)
    return ctxs[0].get_gramian(side)


def allgather_rows(ctxs, side):
    if len(ctxs) == 1:
        return ctxs[0].get_embeddings(side)
    full = ctxs[0].get_embeddings(side)
    for c in ctxs[1:]:
        lo, hi = c.shard_range(side)
        full[lo:hi] = c.get_embeddings(side)[lo:hi]
    for c in ctxs:
        c.set_embeddings(side, full)
    return full
