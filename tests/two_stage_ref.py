"""numpy float64 model of frecsys_recommend_two_stage (include/frecsys_hip.h):
the bf16 rounding, the bound, the certificate, and the fixtures the CPU and GPU
tests share (helper of tests/test_two_stage_cpu.py / test_two_stage_gpu.py).

The model knows nothing of the matrix core's accumulation order: its stage-1
score is the float64 sum of the bf16 products.  Its statements about a fixture
therefore carry a margin: a row "certifies" only when the certificate holds
with 1.01 B, and "cannot certify" only when it fails with 0.99 B, so that
neither statement depends on the last bits of an fp32 accumulator.
"""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)

# (dim, rows, items, k, pool): Dh != Dp (8); unpadded and padded dims; both
# wide widths; row counts that are no multiple of 64; one tile minus one item
# (127); several tiles with a tail (300, 1000); candidate buffers of 512 and
# 2048 slots (pool 64 / 128, and 400)
FIXTURES = (
    (8, 33, 300, 10, 64),
    (20, 70, 127, 10, 64),
    (100, 70, 1000, 10, 64),
    (256, 70, 1000, 20, 128),
    (256, 70, 1000, 100, 400),
    (300, 33, 1000, 10, 64),
    (1000, 33, 1000, 10, 128),
    # padded widths 96, 160, 224: 12, 20, 28 granules, no whole number of the
    # scan's 8-granule k-slabs
    (96, 70, 300, 10, 64),
    (150, 33, 1000, 10, 64),
    (224, 70, 300, 10, 64),
)
NEAR_TIE = (64, 33, 1000, 10, 64)
CANCEL = ((256, 33, 300, 10, 64), (1000, 33, 300, 10, 64))


def padded_dim(dim):
    """frecsys_padded_dim: 8, 16, multiples of 32 up to 256, then 512 and 1024."""
    if dim < 1 or dim > 1024:
        return 0
    if dim <= 8:
        return 8
    if dim <= 16:
        return 16
    if dim <= 256:
        return (dim + 31) // 32 * 32
    return 512 if dim <= 512 else 1024


def bf16_round(x):
    """Round-to-nearest-even to bf16 on the bit pattern, widened back to fp32;
    a NaN stays a NaN (quiet, its upper payload kept)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, ((u >> 16) | 0x40) << 16, r)
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def c_of(dp):
    return 2.0 ** -7 + 2.0 ** -16 + 3.0 * dp * 2.0 ** -23


def bound(dim, query_norm, item_norm_max):
    """B = (c(Dp) ||x||) N in double."""
    return c_of(padded_dim(dim)) * np.float64(query_norm) * np.float64(item_norm_max)


def tables(dim, rows, items, seed):
    """(U [rows, dim], V [items, dim]) float32, N(0, 1/dim) per entry."""
    rng = np.random.default_rng(seed)
    s = dim ** -0.5
    return ((s * rng.standard_normal((rows, dim))).astype(np.float32),
            (s * rng.standard_normal((items, dim))).astype(np.float32))


def fixture(i):
    dim, rows, items, k, pool = FIXTURES[i]
    return tables(dim, rows, items, 7100 + i) + (k, pool)


def near_tie():
    """Every item is one base row + 1e-4 noise: the scores of a row differ by
    far less than the bf16 error, so stage 1 cannot tell the items apart."""
    dim, rows, items, k, pool = NEAR_TIE
    rng = np.random.default_rng(7200)
    s = dim ** -0.5
    U = (s * rng.standard_normal((rows, dim))).astype(np.float32)
    base = s * rng.standard_normal(dim)
    V = (base[None, :] + 1e-4 * s * rng.standard_normal((items, dim))).astype(np.float32)
    return U, V, k, pool


def mixed():
    """(U, V, k, pool, certifying): 960 near-tie items and 40 unrelated ones.
    A row along +base scores every near-tie item alike and above the rest: it
    cannot certify.  A row along -base ranks the 40 unrelated items first, a
    whole |base|^2 above the near-tie crowd that fills its pool: it certifies.
    Rows alternate."""
    dim, rows, _, k, pool = NEAR_TIE
    rng = np.random.default_rng(7250)
    s = dim ** -0.5
    base = s * rng.standard_normal(dim)
    V = np.concatenate([base[None, :] + 1e-4 * s * rng.standard_normal((960, dim)),
                        s * rng.standard_normal((40, dim))])
    V = V[rng.permutation(len(V))].astype(np.float32)
    sign = np.where(np.arange(rows) % 2 == 0, -1.0, 1.0)
    U = (sign[:, None] * base[None, :] + 0.05 * s * rng.standard_normal((rows, dim)))
    return U.astype(np.float32), V, k, pool, sign < 0


def cancellation(i):
    """Entries alternating +-2^10 g and g: the large products cancel, so the
    accumulator's rounding is measured against a sum of magnitudes far above
    the score."""
    dim, rows, items, k, pool = CANCEL[i]
    rng = np.random.default_rng(7300 + i)
    s = dim ** -0.5

    def tab(n):
        g = s * rng.standard_normal((n, dim))
        g[:, 0::2] *= 1024.0 * rng.choice((-1.0, 1.0), size=g[:, 0::2].shape)
        return g.astype(np.float32)
    return tab(rows), tab(items), k, pool


def integer_tables(dim, rows, items, seed):
    """Entries in [-4, 4]: bf16-exact, and every sum exact in fp32 in any
    order (|sum| <= 16 dim < 2^24).  Heavy ties."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, (rows, dim)).astype(np.float32),
            rng.integers(-4, 5, (items, dim)).astype(np.float32))


def histories(rows, items, seed, longest=20):
    """A CSR of distinct item ids per row (lengths 0 .. longest)."""
    rng = np.random.default_rng(seed)
    ptr, col = [0], []
    for _ in range(rows):
        h = int(rng.integers(0, longest + 1))
        col += sorted(rng.choice(items, size=min(h, items), replace=False).tolist())
        ptr.append(len(col))
    return np.array(ptr, np.int64), np.array(col, np.int32)


def _order(score, ids):
    """ids sorted by (score descending, id ascending)."""
    return ids[np.lexsort((ids, -score[ids]))]


def model(U, V, k, pool, eligible=None):
    """Per row, in float64: 'in_pool' (the exact top-k lies inside the bf16
    top-pool), 'certifies' (holds with 1.01 B), 'cannot' (fails with 0.99 B),
    and the pools / lists as id arrays.  eligible: bool [rows, items] or None."""
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    S = U64 @ V64.T
    Sh = bf16_round(U).astype(np.float64) @ bf16_round(V).astype(np.float64).T
    nmax = np.sqrt((V64 * V64).sum(1)).max()
    xn = np.sqrt((U64 * U64).sum(1))
    dim = U.shape[1]
    out = {"in_pool": [], "certifies": [], "cannot": [], "pool": [], "list": [], "S": S, "Sh": Sh}
    for r in range(U.shape[0]):
        ids = np.arange(V.shape[0]) if eligible is None else np.flatnonzero(eligible[r])
        pl = _order(Sh[r], ids)[:pool]
        ls = _order(S[r], pl)[:k]
        top = _order(S[r], ids)[:k]
        B = bound(dim, xn[r], nmax)
        if len(pl) < pool:  # (a): every eligible item is re-scored
            cert, cannot = True, False
        else:
            gap = S[r, ls[-1]] - Sh[r, pl[-1]]
            cert, cannot = bool(gap > 1.01 * B), bool(gap < 0.99 * B)
        out["in_pool"].append(bool(np.isin(top, pl).all()))
        out["certifies"].append(cert)
        out["cannot"].append(cannot)
        out["pool"].append(pl)
        out["list"].append(ls)
    return out
