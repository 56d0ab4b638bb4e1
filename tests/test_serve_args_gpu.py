"""The argument checks of the seven ranking / evaluation entry points of a
context (csrc/serve.hip), one call per single defect: the error code and the
message text, and what a call with zero rows answers.

Each entry point checks in an order of its own and returns at zero rows at a
point of its own (frecsys_rank_candidates and the two candidate-metrics calls
answer OK for zero rows before they look at the exclude flag;
frecsys_recommend, frecsys_rank_metrics and frecsys_similar do not), so the
table spells every expectation out.  The calls go to the C-ABI directly: the
Python wrappers cannot express a negative row count, an unknown flag bit or a
null output.

test_defaults_are_valid   the arguments every case starts from succeed.
test_defects     every (entry point, defect) of CASES: code and message.
test_zero_rows   zero rows: valid, exclude without a CSR, a bad k / cut-off.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

NU, NI, DIM = 6, 5, 8
U, E, I = fh.SIDE_USER, fh.SIDE_EVAL, fh.SIDE_ITEM
EXC = fh.REC_EXCLUDE_HISTORY
INVALID = fh.ERR_INVALID


def i64(*v):
    return np.array(v, dtype=np.int64)


def i32(*v):
    return np.array(v, dtype=np.int32)


# Valid arguments of every entry point: two query rows (rows == None: rows 0
# and 1 of the side), no flags, no mask; outputs with room for 8 rows.
def defaults():
    return dict(side=U, rows=None, n=2, k=3, flags=0, mask=None,
                items=np.zeros(8 * 3, np.int32), scores=np.zeros(8 * 3, np.float32),
                recall=np.zeros(8 * 33, np.float32), ndcg=np.zeros(8 * 33, np.float32),
                k_list=i32(1, 3), nk=2, gt_ptr=i64(0, 1, 3), gt_items=i32(2, 0, 4),
                cand_ptr=i64(0, 2, 5), cand_items=i32(1, 3, 0, 2, 4),
                pair_rows=i64(0, 5), pair_items=i32(4, 0), pair_out=np.zeros(2, np.float32),
                n_neg=2, seed=7, neg_count=None, negatives=None)


P = fh._ptr


def recommend(c, a):
    return c.lib.frecsys_recommend(c.h, a["side"], P(a["rows"]), a["n"], a["k"], a["flags"],
                                   P(a["mask"]), P(a["items"]), P(a["scores"]))


def rank_metrics(c, a):
    return c.lib.frecsys_rank_metrics(c.h, a["side"], P(a["rows"]), a["n"], a["flags"],
                                      P(a["mask"]), P(a["gt_ptr"]), P(a["gt_items"]),
                                      P(a["k_list"]), a["nk"], P(a["recall"]), P(a["ndcg"]))


def score_pairs(c, a):
    return c.lib.frecsys_score_pairs(c.h, a["side"], P(a["pair_rows"]), P(a["pair_items"]),
                                     a["n"], P(a["pair_out"]))


def rank_candidates(c, a):
    return c.lib.frecsys_rank_candidates(c.h, a["side"], P(a["rows"]), a["n"], P(a["cand_ptr"]),
                                         P(a["cand_items"]), a["k"], a["flags"], P(a["mask"]),
                                         P(a["items"]), P(a["scores"]))


def rank_candidates_metrics(c, a):
    return c.lib.frecsys_rank_candidates_metrics(
        c.h, a["side"], P(a["rows"]), a["n"], P(a["cand_ptr"]), P(a["cand_items"]), a["flags"],
        P(a["mask"]), P(a["gt_ptr"]), P(a["gt_items"]), P(a["k_list"]), a["nk"], P(a["recall"]),
        P(a["ndcg"]))


def sampled_metrics(c, a):
    return c.lib.frecsys_sampled_metrics(
        c.h, a["side"], P(a["rows"]), a["n"], a["flags"], P(a["mask"]), P(a["gt_ptr"]),
        P(a["gt_items"]), a["n_neg"], a["seed"], P(a["k_list"]), a["nk"], P(a["recall"]),
        P(a["ndcg"]), P(a["neg_count"]), P(a["negatives"]))


def similar(c, a):
    return c.lib.frecsys_similar(c.h, a["side"], P(a["rows"]), a["n"], a["k"], a["flags"],
                                 P(a["mask"]), P(a["items"]), P(a["scores"]))


# seven rows for a side of six: pointer arrays of eight entries
PTR7 = i64(0, 1, 2, 3, 4, 5, 6, 7)
IDS7 = i32(0, 1, 2, 3, 4, 0, 1)
MORE_ROWS = dict(n=7, gt_ptr=PTR7, gt_items=IDS7, cand_ptr=PTR7, cand_items=IDS7)
K33 = np.ones(33, np.int32)

SIDE_UE = "side must be USER or EVAL"
K_RANGE = "k must be in [1, 1024]"
NULL_OUT = "bad arguments (null outputs)"
NO_CSR = "exclude flag on a side with no CSR loaded"
MORE = "more rows than the side has"
NEG_ROWS = "negative row count"
HOLD = "k_list must hold 1 to 32 cut-offs"
CUT_RANGE = "cut-offs must be in [1, 1024]"
NO_GT = "row 1 has no ground truth"
GT_RANGE = "ground-truth id 5 out of range"

# (entry point, message prefix, defect, argument overrides, context, message);
# the context is "csr" (USER CSR loaded) or "bare" (no CSR); the code is
# FRECSYS_ERR_INVALID throughout.
CASES = [
    (recommend, "recommend", "wrong side", dict(side=I), "csr", SIDE_UE),
    (recommend, "recommend", "k = 0", dict(k=0), "csr", K_RANGE),
    (recommend, "recommend", "k = 1025", dict(k=1025), "csr", K_RANGE),
    (recommend, "recommend", "unknown flag", dict(flags=2), "csr", "unknown flag"),
    (recommend, "recommend", "negative rows", dict(n=-1), "csr", NULL_OUT),
    (recommend, "recommend", "null items", dict(items=None), "csr", NULL_OUT),
    (recommend, "recommend", "exclude, no CSR", dict(flags=EXC), "bare", NO_CSR),
    (recommend, "recommend", "row id -1", dict(rows=i64(0, -1)), "csr", "row id -1 out of range"),
    (recommend, "recommend", "row id n", dict(rows=i64(0, NU)), "csr", "row id 6 out of range"),
    (recommend, "recommend", "more rows", MORE_ROWS, "csr", MORE),

    (rank_metrics, "rank_metrics", "wrong side", dict(side=I), "csr", SIDE_UE),
    (rank_metrics, "rank_metrics", "unknown flag", dict(flags=2), "csr", "unknown flag"),
    (rank_metrics, "rank_metrics", "negative rows", dict(n=-1), "csr", NULL_OUT),
    (rank_metrics, "rank_metrics", "null recall", dict(recall=None), "csr", NULL_OUT),
    (rank_metrics, "rank_metrics", "null ndcg", dict(ndcg=None), "csr", NULL_OUT),
    (rank_metrics, "rank_metrics", "exclude, no CSR", dict(flags=EXC), "bare", NO_CSR),
    (rank_metrics, "rank_metrics", "row id -1", dict(rows=i64(-1, 0)), "csr",
     "row id -1 out of range"),
    (rank_metrics, "rank_metrics", "row id n", dict(rows=i64(0, NU)), "csr",
     "row id 6 out of range"),
    (rank_metrics, "rank_metrics", "more rows", MORE_ROWS, "csr", MORE),
    (rank_metrics, "rank_metrics", "no cut-offs", dict(nk=0), "csr", HOLD),
    (rank_metrics, "rank_metrics", "null k_list", dict(k_list=None), "csr", HOLD),
    (rank_metrics, "rank_metrics", "33 cut-offs", dict(k_list=K33, nk=33), "csr", HOLD),
    (rank_metrics, "rank_metrics", "cut-off 0", dict(k_list=i32(1, 0)), "csr", CUT_RANGE),
    (rank_metrics, "rank_metrics", "cut-off 1025", dict(k_list=i32(1025, 1)), "csr", CUT_RANGE),
    (rank_metrics, "rank_metrics", "empty gt row", dict(gt_ptr=i64(0, 1, 1)), "csr", NO_GT),
    (rank_metrics, "rank_metrics", "gt id n_items", dict(gt_items=i32(2, 0, NI)), "csr", GT_RANGE),
    (rank_metrics, "rank_metrics", "gt id -1", dict(gt_items=i32(-1, 0, 4)), "csr",
     "ground-truth id -1 out of range"),
    (rank_metrics, "rank_metrics", "gt_ptr[0]", dict(gt_ptr=i64(1, 2, 3)), "csr",
     "gt_ptr[0] must be 0"),
    (rank_metrics, "rank_metrics", "null gt_ptr", dict(gt_ptr=None), "csr",
     "bad arguments (null gt_ptr / k_list, n < 0)"),

    (score_pairs, "score_pairs", "wrong side", dict(side=I), "csr", SIDE_UE),
    (score_pairs, "score_pairs", "negative pairs", dict(n=-1), "csr", "negative pair count"),
    (score_pairs, "score_pairs", "null rows", dict(pair_rows=None), "csr", "null pointer"),
    (score_pairs, "score_pairs", "null items", dict(pair_items=None), "csr", "null pointer"),
    (score_pairs, "score_pairs", "null scores", dict(pair_out=None), "csr", "null pointer"),
    (score_pairs, "score_pairs", "row id -1", dict(pair_rows=i64(0, -1)), "csr",
     "row id -1 out of range"),
    (score_pairs, "score_pairs", "row id n", dict(pair_rows=i64(NU, 0)), "csr",
     "row id 6 out of range"),
    (score_pairs, "score_pairs", "item id -1", dict(pair_items=i32(-1, 0)), "csr",
     "item id -1 out of range"),
    (score_pairs, "score_pairs", "item id n_items", dict(pair_items=i32(4, NI)), "csr",
     "item id 5 out of range"),

    (rank_candidates, "rank_candidates", "wrong side", dict(side=I), "csr", SIDE_UE),
    (rank_candidates, "rank_candidates", "k = 0", dict(k=0), "csr", K_RANGE),
    (rank_candidates, "rank_candidates", "k = 1025", dict(k=1025), "csr", K_RANGE),
    (rank_candidates, "rank_candidates", "unknown flag", dict(flags=4), "csr", "unknown flag"),
    (rank_candidates, "rank_candidates", "negative rows", dict(n=-1), "csr", NEG_ROWS),
    (rank_candidates, "rank_candidates", "null cand_ptr", dict(cand_ptr=None), "csr",
     "null pointer"),
    (rank_candidates, "rank_candidates", "null items", dict(items=None), "csr", "null pointer"),
    (rank_candidates, "rank_candidates", "exclude, no CSR", dict(flags=EXC), "bare", NO_CSR),
    (rank_candidates, "rank_candidates", "row id -1", dict(rows=i64(-1, 0)), "csr",
     "row id -1 out of range"),
    (rank_candidates, "rank_candidates", "row id n", dict(rows=i64(0, NU)), "csr",
     "row id 6 out of range"),
    (rank_candidates, "rank_candidates", "more rows", MORE_ROWS, "csr", MORE),
    (rank_candidates, "rank_candidates", "cand_ptr[0]", dict(cand_ptr=i64(1, 2, 5)), "csr",
     "cand_ptr[0] must be 0"),
    (rank_candidates, "rank_candidates", "cand_ptr order", dict(cand_ptr=i64(0, 5, 4)), "csr",
     "cand_ptr not monotone at row 1"),
    (rank_candidates, "rank_candidates", "null cand_items", dict(cand_items=None), "csr",
     "null cand_items"),
    (rank_candidates, "rank_candidates", "candidate id n_items",
     dict(cand_items=i32(1, 3, 0, NI, 4)), "csr", "candidate id 5 out of range"),
    (rank_candidates, "rank_candidates", "candidate id -1",
     dict(cand_items=i32(-1, 3, 0, 2, 4)), "csr", "candidate id -1 out of range"),

    (rank_candidates_metrics, "rank_candidates_metrics", "wrong side", dict(side=I), "csr",
     SIDE_UE),
    (rank_candidates_metrics, "rank_candidates_metrics", "unknown flag", dict(flags=2), "csr",
     "unknown flag"),
    (rank_candidates_metrics, "rank_candidates_metrics", "negative rows", dict(n=-1), "csr",
     NEG_ROWS),
    (rank_candidates_metrics, "rank_candidates_metrics", "null cand_ptr", dict(cand_ptr=None),
     "csr", "null cand_ptr"),
    (rank_candidates_metrics, "rank_candidates_metrics", "null recall", dict(recall=None), "csr",
     NULL_OUT),
    (rank_candidates_metrics, "rank_candidates_metrics", "null ndcg", dict(ndcg=None), "csr",
     NULL_OUT),
    (rank_candidates_metrics, "rank_candidates_metrics", "exclude, no CSR", dict(flags=EXC),
     "bare", NO_CSR),
    (rank_candidates_metrics, "rank_candidates_metrics", "row id -1", dict(rows=i64(0, -1)),
     "csr", "row id -1 out of range"),
    (rank_candidates_metrics, "rank_candidates_metrics", "row id n", dict(rows=i64(NU, 0)),
     "csr", "row id 6 out of range"),
    (rank_candidates_metrics, "rank_candidates_metrics", "more rows", MORE_ROWS, "csr", MORE),
    (rank_candidates_metrics, "rank_candidates_metrics", "no cut-offs", dict(nk=0), "csr", HOLD),
    (rank_candidates_metrics, "rank_candidates_metrics", "null k_list", dict(k_list=None), "csr",
     HOLD),
    (rank_candidates_metrics, "rank_candidates_metrics", "33 cut-offs", dict(k_list=K33, nk=33),
     "csr", HOLD),
    (rank_candidates_metrics, "rank_candidates_metrics", "cut-off 0", dict(k_list=i32(0, 3)),
     "csr", CUT_RANGE),
    (rank_candidates_metrics, "rank_candidates_metrics", "cut-off 1025",
     dict(k_list=i32(1, 1025)), "csr", CUT_RANGE),
    (rank_candidates_metrics, "rank_candidates_metrics", "empty gt row",
     dict(gt_ptr=i64(0, 1, 1)), "csr", NO_GT),
    (rank_candidates_metrics, "rank_candidates_metrics", "gt id n_items",
     dict(gt_items=i32(2, 0, NI)), "csr", GT_RANGE),
    (rank_candidates_metrics, "rank_candidates_metrics", "cand_ptr[0]",
     dict(cand_ptr=i64(1, 2, 5)), "csr", "cand_ptr[0] must be 0"),
    (rank_candidates_metrics, "rank_candidates_metrics", "cand_ptr order",
     dict(cand_ptr=i64(0, 5, 4)), "csr", "cand_ptr not monotone at row 1"),
    (rank_candidates_metrics, "rank_candidates_metrics", "null cand_items",
     dict(cand_items=None), "csr", "null cand_items"),
    (rank_candidates_metrics, "rank_candidates_metrics", "candidate id n_items",
     dict(cand_items=i32(1, 3, 0, NI, 4)), "csr", "candidate id 5 out of range"),

    (sampled_metrics, "sampled_metrics", "wrong side", dict(side=I), "csr", SIDE_UE),
    (sampled_metrics, "sampled_metrics", "unknown flag", dict(flags=2), "csr", "unknown flag"),
    (sampled_metrics, "sampled_metrics", "negative rows", dict(n=-1), "csr", NEG_ROWS),
    (sampled_metrics, "sampled_metrics", "negative n_neg", dict(n_neg=-1), "csr",
     "n_neg must not be negative"),
    (sampled_metrics, "sampled_metrics", "null recall", dict(recall=None), "csr", NULL_OUT),
    (sampled_metrics, "sampled_metrics", "exclude, no CSR", dict(flags=EXC), "bare", NO_CSR),
    (sampled_metrics, "sampled_metrics", "row id -1", dict(rows=i64(-1, 0)), "csr",
     "row id -1 out of range"),
    (sampled_metrics, "sampled_metrics", "row id n", dict(rows=i64(0, NU)), "csr",
     "row id 6 out of range"),
    (sampled_metrics, "sampled_metrics", "more rows", MORE_ROWS, "csr", MORE),
    (sampled_metrics, "sampled_metrics", "no cut-offs", dict(nk=0), "csr", HOLD),
    (sampled_metrics, "sampled_metrics", "33 cut-offs", dict(k_list=K33, nk=33), "csr", HOLD),
    (sampled_metrics, "sampled_metrics", "cut-off 0", dict(k_list=i32(3, 0)), "csr", CUT_RANGE),
    (sampled_metrics, "sampled_metrics", "cut-off 1025", dict(k_list=i32(1025, 3)), "csr",
     CUT_RANGE),
    (sampled_metrics, "sampled_metrics", "empty gt row", dict(gt_ptr=i64(0, 1, 1)), "csr", NO_GT),
    (sampled_metrics, "sampled_metrics", "gt id n_items", dict(gt_items=i32(2, 0, NI)), "csr",
     GT_RANGE),

    (similar, "similar", "wrong side", dict(side=E), "csr", "side must be USER or ITEM"),
    (similar, "similar", "k = 0", dict(k=0), "csr", K_RANGE),
    (similar, "similar", "k = 1025", dict(k=1025), "csr", K_RANGE),
    (similar, "similar", "unknown flag", dict(flags=4), "csr", "unknown flag"),
    (similar, "similar", "negative rows", dict(n=-1), "csr", NULL_OUT),
    (similar, "similar", "null ids", dict(items=None), "csr", NULL_OUT),
    (similar, "similar", "row id -1", dict(rows=i64(0, -1)), "csr", "row id -1 out of range"),
    (similar, "similar", "row id n", dict(rows=i64(NU, 0)), "csr", "row id 6 out of range"),
    (similar, "similar", "row id n of the items", dict(side=I, rows=i64(0, NI)), "csr",
     "row id 5 out of range"),
    (similar, "similar", "more rows", dict(n=7), "csr", MORE),
]

# Zero rows: (entry point, prefix, state, overrides, context, None = OK or the
# message of FRECSYS_ERR_INVALID).  score_pairs has neither flags nor k: its
# states are valid, null pointers and a wrong side.
ZERO = [
    (recommend, "recommend", "valid", dict(), "csr", None),
    (recommend, "recommend", "exclude, no CSR", dict(flags=EXC), "bare", NO_CSR),
    (recommend, "recommend", "k = 0", dict(k=0), "csr", K_RANGE),
    (rank_metrics, "rank_metrics", "valid", dict(gt_ptr=i64(0)), "csr", None),
    (rank_metrics, "rank_metrics", "exclude, no CSR", dict(gt_ptr=i64(0), flags=EXC), "bare",
     NO_CSR),
    (rank_metrics, "rank_metrics", "cut-off 0", dict(gt_ptr=i64(0), k_list=i32(0, 3)), "csr",
     CUT_RANGE),
    (score_pairs, "score_pairs", "valid", dict(), "csr", None),
    (score_pairs, "score_pairs", "null pointers",
     dict(pair_rows=None, pair_items=None, pair_out=None), "csr", None),
    (score_pairs, "score_pairs", "wrong side", dict(side=I), "csr", SIDE_UE),
    (rank_candidates, "rank_candidates", "valid", dict(cand_ptr=i64(0)), "csr", None),
    (rank_candidates, "rank_candidates", "exclude, no CSR", dict(cand_ptr=i64(0), flags=EXC),
     "bare", None),
    (rank_candidates, "rank_candidates", "k = 1025", dict(cand_ptr=i64(0), k=1025), "csr",
     K_RANGE),
    (rank_candidates_metrics, "rank_candidates_metrics", "valid",
     dict(cand_ptr=i64(0), gt_ptr=i64(0)), "csr", None),
    (rank_candidates_metrics, "rank_candidates_metrics", "null cand_ptr",
     dict(cand_ptr=None, gt_ptr=None), "csr", None),
    (rank_candidates_metrics, "rank_candidates_metrics", "exclude, no CSR",
     dict(cand_ptr=i64(0), gt_ptr=i64(0), flags=EXC), "bare", None),
    (rank_candidates_metrics, "rank_candidates_metrics", "cut-off 0",
     dict(cand_ptr=i64(0), gt_ptr=i64(0), k_list=i32(1, 0)), "csr", CUT_RANGE),
    (sampled_metrics, "sampled_metrics", "valid", dict(gt_ptr=i64(0)), "csr", None),
    (sampled_metrics, "sampled_metrics", "exclude, no CSR", dict(gt_ptr=i64(0), flags=EXC),
     "bare", None),
    (sampled_metrics, "sampled_metrics", "cut-off 1025", dict(gt_ptr=i64(0), k_list=i32(1025, 1)),
     "csr", CUT_RANGE),
    (sampled_metrics, "sampled_metrics", "negative n_neg", dict(gt_ptr=i64(0), n_neg=-1), "csr",
     "n_neg must not be negative"),
    (similar, "similar", "valid", dict(), "csr", None),
    (similar, "similar", "k = 0", dict(k=0), "csr", K_RANGE),
    (similar, "similar", "unknown flag", dict(flags=8), "csr", "unknown flag"),
]


@pytest.fixture(scope="module")
def contexts():
    ptr = i64(0, 1, 3, 3, 4, 6, 7)
    col = i32(2, 0, 4, 1, 0, 3, 2)
    with fh.Context(DIM, NU, NI) as csr, fh.Context(DIM, NU, NI) as bare:
        csr.load_csr(U, ptr, col)
        csr.init_embeddings(11, 0.1)
        bare.init_embeddings(11, 0.1)
        yield {"csr": csr, "bare": bare}


def _ids(table):
    return [f"{t[1]}-{t[2]}".replace(" ", "_") for t in table]


def _run(contexts, fn, over, which):
    args = defaults()
    args.update(over)
    ctx = contexts[which]
    ctx._check(fn(ctx, args))


ENTRY_POINTS = [recommend, rank_metrics, score_pairs, rank_candidates, rank_candidates_metrics,
                sampled_metrics, similar]


@pytest.mark.parametrize("fn", ENTRY_POINTS, ids=[f.__name__ for f in ENTRY_POINTS])
def test_defaults_are_valid(contexts, fn):
    # so that each case of CASES has its one defect only; also on the context
    # without a CSR, and with the exclude flag where one is loaded
    _run(contexts, fn, {}, "csr")
    _run(contexts, fn, {}, "bare")
    _run(contexts, fn, dict(flags=EXC if fn is not similar else 0), "csr")


@pytest.mark.parametrize("fn,prefix,defect,over,which,msg", CASES, ids=_ids(CASES))
def test_defects(contexts, fn, prefix, defect, over, which, msg):
    with pytest.raises(fh.FrecsysError) as e:
        _run(contexts, fn, over, which)
    assert e.value.code == INVALID, e.value
    assert str(e.value) == f"frecsys error {INVALID}: {prefix}: {msg}"


@pytest.mark.parametrize("fn,prefix,state,over,which,msg", ZERO, ids=_ids(ZERO))
def test_zero_rows(contexts, fn, prefix, state, over, which, msg):
    over = dict(over, n=0)
    if msg is None:
        _run(contexts, fn, over, which)
        return
    with pytest.raises(fh.FrecsysError) as e:
        _run(contexts, fn, over, which)
    assert e.value.code == INVALID, e.value
    assert str(e.value) == f"frecsys error {INVALID}: {prefix}: {msg}"
