"""Pure-Python restatement of the sampled-evaluation definitions of
include/frecsys_hip.h (frecsys_sample_negatives), and the fixtures of
tests/test_sampled_cpu.py, tests/test_sampled_gpu.py and
tests/test_sampled_model_gpu.py (a helper, not a test).  It does not import
the library.

sample()        neg_count / negatives of every query row, draw by draw, plus
                what the draws met: E, M, whole-pool flags, and the repeats of
                an accepted id inside its block of 64 draws and across blocks.
pool_of()       the pool of a row as ascending ids.
lists_from()    the candidate lists (distinct ground truth, then negatives or
                the whole pool) of a sampler's outputs.
histories() / ground_truth() / mask_of() / row_ids() / plan()
                the inputs of the grids.
"""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
CAP_BASE, CAP_PER_NEG = 1 << 20, 4096

GRID_ITEMS = (1, 2, 129, 5000)
GRID_NEG = (0, 1, 63, 64, 65, 100, 1000)
GRID_MASKS = ("none", "m70", "single", "zero")
GRID_SEEDS = (0, 1, MASK64)
GRID_ROWMODES = ("none", "shuffled", "ordered")


def mix64(x):
    x &= MASK64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    x ^= x >> 31
    return x


def whole_pool(n_neg, E, M):
    return 2 * n_neg > E or 64 * E < M


def sample(n_items, mask, rows, hist, gt_ptr, gt_items, n_neg, seed):
    """rows: side row id per query row, or None; hist: (ptr, items) per query
    row, or None.  Returns a dict: neg_count, negatives ([n, n_neg], -1 rows
    for whole-pool rows), E, M, whole, in_block, across_blocks (counts of
    draws rejected as a repeat of a draw accepted in the same / an earlier
    block of 64), draws."""
    n = len(gt_ptr) - 1
    D = list(range(n_items)) if mask is None else [j for j in range(n_items) if mask[j]]
    M = len(D)
    inD = set(D)
    cnt = np.zeros(n, np.int32)
    neg = np.full((n, n_neg), -1, np.int32)
    Es, whole = [], []
    in_block = across = draws = 0
    for i in range(n):
        r = i if rows is None else int(rows[i])
        blocked = set(int(j) for j in gt_items[gt_ptr[i]:gt_ptr[i + 1]])
        if hist is not None:
            blocked |= set(int(j) for j in hist[1][hist[0][i]:hist[0][i + 1]])
        E = M - len(blocked & inD)
        Es.append(E)
        whole.append(whole_pool(n_neg, E, M))
        if whole[-1]:
            cnt[i] = E
            continue
        cnt[i] = n_neg
        key = mix64(seed + GOLDEN * (r + 1))
        taken = {}
        t = 0
        while len(taken) < n_neg:
            assert t < CAP_BASE + CAP_PER_NEG * n_neg
            u = mix64(key + GOLDEN * (t + 1))
            j = D[((u >> 32) * M) >> 32]
            if j in taken:
                if taken[j] // 64 == t // 64:
                    in_block += 1
                else:
                    across += 1
            elif j not in blocked:
                neg[i, len(taken)] = j
                taken[j] = t
            t += 1
        draws += t
    return {"neg_count": cnt, "negatives": neg, "E": np.array(Es), "M": M,
            "whole": np.array(whole, bool), "in_block": in_block, "across_blocks": across,
            "draws": draws}


def pool_of(n_items, mask, hist_row, gt_row):
    ok = np.ones(n_items, bool) if mask is None else np.asarray(mask) != 0
    ok = ok.copy()
    ok[np.asarray(gt_row, np.int64)] = False
    h = np.asarray(hist_row, np.int64)
    ok[h[(h >= 0) & (h < n_items)]] = False
    return np.nonzero(ok)[0].astype(np.int32)


def lists_from(n_items, mask, hist, gt_ptr, gt_items, n_neg, neg_count, negatives):
    """(cand_ptr, cand_items) of a sampler's outputs: row i = its distinct
    ground truth ascending, then its negatives -- its whole pool where the
    sampler says so (a count other than n_neg, or a -1 row)."""
    out = []
    for i in range(len(gt_ptr) - 1):
        g = np.unique(gt_items[gt_ptr[i]:gt_ptr[i + 1]]).astype(np.int32)
        if neg_count[i] != n_neg or (n_neg > 0 and negatives[i, 0] == -1):
            h = hist[1][hist[0][i]:hist[0][i + 1]] if hist is not None else []
            ng = pool_of(n_items, mask, h, g)
            assert len(ng) == neg_count[i]
        else:
            ng = negatives[i]
        out.append(np.concatenate([g, ng]).astype(np.int32))
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in out])]).astype(np.int64)
    return ptr, np.concatenate(out).astype(np.int32)


def mask_of(n_items, kind, seed):
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros(n_items, np.uint8)
    if kind == "single":
        m = np.zeros(n_items, np.uint8)
        m[(7 * seed + n_items // 2) % n_items] = 1
        return m
    return (np.random.default_rng(seed + 2).random(n_items) < 0.7).astype(np.uint8)


def histories(n_rows, n_items, seed):
    """CSR histories: row 0 empty, row 1 {0, n_items - 1}, row 2 with repeated
    ids, row 3 all but 3 items (a pool below 1/64 of a large catalogue), row 4
    half of the items, the others 1 .. 40 distinct ids."""
    rng = np.random.default_rng(seed)
    hs = []
    for r in range(n_rows):
        if r == 0:
            h = []
        elif r == 1:
            h = [0, n_items - 1]
        elif r == 2:
            a = rng.integers(0, n_items, 6)
            h = np.concatenate([a, a[:3]])
        elif r == 3:
            h = rng.permutation(n_items)[:max(n_items - 3, 0)]
        elif r == 4:
            h = rng.permutation(n_items)[:n_items // 2]
        else:
            h = rng.permutation(n_items)[:min(n_items, int(rng.integers(1, 41)))]
        hs.append(np.asarray(h, np.int32))
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int64)
    col = np.concatenate(hs).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, col


def ground_truth(n_rows, n_items, hist, mask, seed):
    """A list of rows: 1 .. 8 ids each with a repeat now and then; where there
    is one, an id of the row's history and a masked-out id are among them."""
    rng = np.random.default_rng(seed)
    off = None if mask is None else np.nonzero(np.asarray(mask) == 0)[0]
    gs = []
    for i in range(n_rows):
        g = list(rng.integers(0, n_items, int(rng.integers(1, 9))))
        if i % 3 == 0 and len(g) > 1:
            g[-1] = g[0]
        if hist is not None and i % 2 == 1 and hist[0][i + 1] > hist[0][i]:
            g.append(int(hist[1][hist[0][i]]))
        if off is not None and len(off) and i % 4 == 2:
            g.append(int(off[i % len(off)]))
        gs.append(np.asarray(g, np.int32))
    return gs


def csr(lists):
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in lists])]).astype(np.int64)
    col = np.concatenate(lists).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, col


def row_ids(n_rows, n_side, mode, seed):
    """None, or side row ids: shuffled with repeats, or ascending."""
    if mode == "none":
        return None
    rng = np.random.default_rng(seed + 5)
    r = rng.integers(0, n_side, n_rows).astype(np.int64)
    if n_rows >= 4:
        r[n_rows // 2] = r[0]
        r[-1] = r[1]
    return np.sort(r) if mode == "ordered" else r


def plan(items=GRID_ITEMS):
    """(n_items, n_neg, mask kind, with history, seed, row mode, fixture seed):
    every (items, n_neg) pair and every (items, mask) pair; history, seed and
    row mode rotated so that each value meets each item count."""
    out = []
    for a, m in enumerate(items):
        for b, n_neg in enumerate(GRID_NEG):
            out.append((m, n_neg, GRID_MASKS[(a + b) % 4], bool((a + b // 2) % 2),
                        GRID_SEEDS[(a + 2 * b) % 3], GRID_ROWMODES[(a + b) % 3], 100 * a + b))
        for c, mk in enumerate(GRID_MASKS):
            out.append((m, (65, 100, 1, 1000)[c], mk, bool((a + c) % 2), GRID_SEEDS[(a + c) % 3],
                        GRID_ROWMODES[(a + c + 1) % 3], 100 * a + 50 + c))
    return out


def case(n_items, n_rows, mk, with_hist, row_mode, fseed, n_side=None, side_seed=None):
    """(mask, rows, hist per query row, gt_ptr, gt_items, side histories): the
    side has n_side rows (default n_rows) with histories() of side_seed
    (default fseed); query row i is side row rows[i] and carries that row's
    history."""
    n_side = n_rows if n_side is None else n_side
    mask = mask_of(n_items, mk, fseed)
    rows = row_ids(n_rows, n_side, row_mode, fseed)
    side = histories(n_side, n_items, (fseed if side_seed is None else side_seed) + 1)
    hist = None
    if with_hist:
        idx = np.arange(n_rows) if rows is None else rows
        hs = [side[1][side[0][r]:side[0][r + 1]] for r in idx]
        hp = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int64)
        hist = (hp, np.concatenate(hs).astype(np.int32) if hp[-1] else np.zeros(0, np.int32))
    gs = ground_truth(n_rows, n_items, hist, mask, fseed + 3)
    if rows is not None and n_rows >= 4:   # the repeated side rows of row_ids(): equal inputs
        gs[n_rows // 2], gs[-1] = gs[0], gs[1]
    gp, gi = csr(gs)
    return mask, rows, hist, gp, gi, side
