"""The argument checks of the query entry points of a model
(include/frecsys_model.h, tools/model_capi.cc), one call per single defect:
the error code and the message text, what a call with zero rows answers, what
a serve-only model refuses, and that a rejected fold-in call projects nothing.

A defect the model layer checks itself is reported under the entry point's
own name; one it leaves to the context arrives as the context's message
(frecsys_last_error of the model's context) through frecsys_model_last_error:
the trained forms of recommend and rank_candidates leave k, the outputs and the
candidate CSR to it, their fold-in forms check them before they project.  Only
single defects are pinned: which of several wins is not part of the contract.
The calls go to the C-ABI directly: the Python wrappers cannot express a null
output or a negative row count.

test_defaults_are_valid  the arguments every case starts from succeed.
test_defects      every (entry point, defect) of CASES: code and message.
test_zero_rows    zero rows: the answer, and whether `summary` is written.
test_serve_only   a model loaded without tuples: what it refuses, what works.
test_checks_come_before_the_projection  a rejected fold-in leaves EVAL alone.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

fh = pytest.importorskip("frecsys_hip")

NU, NI, DIM = 6, 5, 8
INVALID = fh.ERR_INVALID
SENTINEL = -7.0
P = fh._ptr

# a dozen tuples: every user and every item has a history
TRAIN_USERS = np.array([0, 0, 1, 1, 2, 3, 3, 4, 4, 5, 5, 5], dtype=np.int32)
TRAIN_ITEMS = np.array([2, 0, 0, 4, 1, 1, 3, 0, 3, 2, 4, 1], dtype=np.int32)


def i64(*v):
    return np.array(v, dtype=np.int64)


def i32(*v):
    return np.array(v, dtype=np.int32)


def f32(*v):
    return np.array(v, dtype=np.float32)


# Valid arguments of every entry point: two query rows (trained users 0 and 5,
# or two histories), no exclusion, no mask; outputs with room for 8 rows.
def defaults():
    return dict(model="h", users=i64(0, 5), hist_ptr=i64(0, 2, 3), hist_items=i32(1, 3, 0), n=2,
                k=3, exc=0, mask=None, items=np.zeros(8 * 3, np.int32),
                scores=np.zeros(8 * 3, np.float32),
                cand_ptr=i64(0, 2, 5), cand_items=i32(1, 3, 0, 2, 4),
                gt_ptr=i64(0, 1, 3), gt_items=i32(2, 0, 4), k_list=i32(1, 3), nk=2,
                alpha=f32(0.5), na=1, recall=np.zeros(8 * 33, np.float32),
                ndcg=np.zeros(8 * 33, np.float32), summary=np.full(4 * 33, SENTINEL, np.float32),
                n_neg=2, seed=7, rank=np.zeros(8, np.int32), eligible=np.zeros(8, np.int32),
                mrr=np.zeros(8, np.float32), auc=np.zeros(8, np.float32),
                tgt_ptr=i64(0, 1, 3), tgt_items=i32(2, 0, 4), top=2,
                score=np.zeros(8, np.float32), top_items=np.zeros(8 * 2, np.int32),
                top_contrib=np.zeros(8 * 2, np.float32), full=None,
                pool=4, lam=0.5, raw=0, mmr=None,
                pair_items=i32(4, 0), pair_out=np.zeros(2, np.float32),
                sim_rows=i64(0, 4), sim_flags=0,
                lists=i32(0, 1, 2, 3, 4, 3, 2, -1), list_scores=f32(4, 3, 2, 1, 4, 3, 2, 0))


# The arguments after the query rows, per entry point.
TAILS = {
    "recommend": lambda a: [a["k"], a["exc"], P(a["mask"]), P(a["items"]), P(a["scores"])],
    "recommend_diverse": lambda a: [a["k"], a["pool"], a["lam"], a["raw"], a["exc"], P(a["mask"]),
                                    P(a["items"]), P(a["scores"]), P(a["mmr"])],
    "explain": lambda a: [P(a["tgt_ptr"]), P(a["tgt_items"]), a["top"], P(a["score"]),
                          P(a["top_items"]), P(a["top_contrib"]), P(a["full"])],
    "rank_candidates": lambda a: [P(a["cand_ptr"]), P(a["cand_items"]), a["k"], a["exc"],
                                  P(a["mask"]), P(a["items"]), P(a["scores"])],
    "evaluate": lambda a: [P(a["gt_ptr"]), P(a["gt_items"]), P(a["k_list"]), a["nk"],
                           P(a["alpha"]), a["na"], a["exc"], P(a["recall"]), P(a["ndcg"]),
                           P(a["summary"])],
    "evaluate_candidates": lambda a: [P(a["cand_ptr"]), P(a["cand_items"]), P(a["gt_ptr"]),
                                      P(a["gt_items"]), P(a["k_list"]), a["nk"], P(a["alpha"]),
                                      a["na"], a["exc"], P(a["mask"]), P(a["recall"]),
                                      P(a["ndcg"]), P(a["summary"])],
    "evaluate_sampled": lambda a: [P(a["gt_ptr"]), P(a["gt_items"]), a["n_neg"], a["seed"],
                                   P(a["k_list"]), a["nk"], P(a["alpha"]), a["na"], a["exc"],
                                   P(a["mask"]), P(a["recall"]), P(a["ndcg"]), P(a["summary"])],
    "evaluate_ranks": lambda a: [P(a["gt_ptr"]), P(a["gt_items"]), P(a["alpha"]), a["na"],
                                 a["exc"], P(a["mask"]), P(a["rank"]), P(a["eligible"]),
                                 P(a["mrr"]), P(a["auc"]), P(a["summary"])],
}
PAIRS = list(TAILS)
# The entry points on trained rows only: the whole argument list after the model.
SINGLES = {
    "score": lambda a: [P(a["users"]), P(a["pair_items"]), a["n"], P(a["pair_out"])],
    "similar_items": lambda a: [P(a["sim_rows"]), a["n"], a["k"], a["sim_flags"], P(a["mask"]),
                                P(a["items"]), P(a["scores"])],
    "similar_users": lambda a: [P(a["users"]), a["n"], a["k"], a["sim_flags"], P(a["mask"]),
                                P(a["items"]), P(a["scores"])],
    "diversify": lambda a: [P(a["lists"]), P(a["list_scores"]), a["n"], a["pool"], a["k"],
                            a["lam"], a["raw"], P(a["items"]), P(a["scores"]), P(a["mmr"])],
}
ENTRY_POINTS = ([(name, fold) for name in PAIRS for fold in (False, True)] +
                [(name, False) for name in SINGLES])


def symbol(name, fold):
    return "frecsys_model_" + name + ("_fold_in" if fold else "")


def call(model, name, fold, over):
    """The status of one call of entry point `name` (its _fold_in form) on
    `model` with the defaults changed by `over`, and the arguments used."""
    a = defaults()
    a.update(over)
    h = model.h if a["model"] == "h" else None
    if name in SINGLES:
        args = SINGLES[name](a)
    elif fold:
        args = [P(a["hist_ptr"]), P(a["hist_items"]), a["n"]] + TAILS[name](a)
    else:
        args = [P(a["users"]), a["n"]] + TAILS[name](a)
    return getattr(model.lib, symbol(name, fold))(h, *args), a


def run(model, name, fold, over):
    rc, a = call(model, name, fold, over)
    if rc:
        raise fh.FrecsysError(rc, model.lib.frecsys_model_last_error().decode())
    return a


K33 = np.ones(33, np.int32)
BAD = "bad arguments"
BAD_GT = "bad arguments (n < 0, gt_ptr)"
HOLD = "k_list must hold 1 to 32 cut-offs"
CUT_RANGE = "cut-offs must be in [1, 1024]"
K_ITEMS = "k must be in [1, 1024], items non-null"
NO_GT = "gt_ptr not monotone or no ground truth at row 1"
NULL_EVAL = "null gt_items / recall / ndcg"

# What the context calls its entry point when a defect is left to it.
CONTEXT = {"recommend": "recommend", "recommend_diverse": "recommend_diverse",
           "explain": "explain", "rank_candidates": "rank_candidates",
           "evaluate": "rank_metrics", "evaluate_candidates": "rank_candidates_metrics",
           "evaluate_sampled": "sampled_metrics", "evaluate_ranks": "rank_positions",
           "score": "score_pairs", "similar_items": "similar", "similar_users": "similar"}
EVALS = ("evaluate", "evaluate_candidates", "evaluate_sampled", "evaluate_ranks")


def trained_rows(name):
    """The defects of the trained rows: (defect, overrides, own message or
    None, context message or None)."""
    neg = BAD_GT if name in EVALS else BAD
    return [("null model", dict(model=None), BAD, None),
            ("negative n", dict(n=-1), neg, None),
            ("null users", dict(users=None), BAD, None),
            ("user id -1", dict(users=i64(-1, 0)), None, "row id -1 out of range"),
            ("user id n_users", dict(users=i64(0, NU)), None, "row id 6 out of range")]


def history_rows():
    return [("null model", dict(model=None), BAD, None),
            ("negative n", dict(n=-1), BAD, None),
            ("null hist_ptr", dict(hist_ptr=None), BAD, None),
            ("hist_ptr[0]", dict(hist_ptr=i64(1, 2, 3)), BAD, None),
            ("hist_ptr order", dict(hist_ptr=i64(0, 3, 2)), "hist_ptr not monotone", None),
            ("null hist_items", dict(hist_items=None), "null hist_items", None),
            ("history id -1", dict(hist_items=i32(1, -1, 0)), "item id -1 out of range", None),
            ("history id n_items", dict(hist_items=i32(1, 3, NI)), "item id 5 out of range", None)]


# The ground-truth, cut-off and alpha defects of the Recall / NDCG evaluations.
TRUTH = [("null gt_ptr", dict(gt_ptr=None), BAD_GT, None),
         ("gt_ptr[0]", dict(gt_ptr=i64(1, 2, 3)), BAD_GT, None),
         ("empty gt row", dict(gt_ptr=i64(0, 1, 1)), NO_GT, None),
         ("gt id -1", dict(gt_items=i32(-1, 0, 4)), "ground-truth id -1 out of range", None),
         ("gt id n_items", dict(gt_items=i32(2, 0, NI)), "ground-truth id 5 out of range", None),
         ("negative na", dict(na=-1), "bad alpha_list", None),
         ("null alpha_list", dict(alpha=None), "bad alpha_list", None)]
METRICS = TRUTH + [
    ("null gt_items", dict(gt_items=None), NULL_EVAL, None),
    ("no cut-offs", dict(nk=0), HOLD, None),
    ("33 cut-offs", dict(k_list=K33, nk=33), HOLD, None),
    ("null k_list", dict(k_list=None), HOLD, None),
    ("cut-off 0", dict(k_list=i32(1, 0)), CUT_RANGE, None),
    ("cut-off 1025", dict(k_list=i32(1025, 1)), CUT_RANGE, None),
    ("null recall", dict(recall=None), NULL_EVAL, None),
    ("null ndcg", dict(ndcg=None), NULL_EVAL, None)]
CANDIDATES = [("null cand_ptr", dict(cand_ptr=None), "bad cand_ptr", None),
              ("cand_ptr[0]", dict(cand_ptr=i64(1, 2, 5)), "bad cand_ptr", None),
              ("cand_ptr order", dict(cand_ptr=i64(0, 5, 4)), "cand_ptr not monotone", None),
              ("null cand_items", dict(cand_items=None), "null cand_items", None),
              ("candidate id -1", dict(cand_items=i32(-1, 3, 0, 2, 4)),
               "candidate id -1 out of range", None),
              ("candidate id n_items", dict(cand_items=i32(1, 3, 0, NI, 4)),
               "candidate id 5 out of range", None)]
RANKS = TRUTH + [
    ("null gt_items", dict(gt_items=None), "null gt_items", None),
    ("null outputs", dict(rank=None, eligible=None, mrr=None, auc=None, summary=None),
     "null outputs", None),
    ("summary without mrr", dict(mrr=None), "summary needs mrr and auc", None),
    ("summary without auc", dict(auc=None), "summary needs mrr and auc", None)]
DIVERSE = [("pool 0", dict(pool=0), "pool must be in [1, 1024]", None),
           ("pool 1025", dict(pool=1025), "pool must be in [1, 1024]", None),
           ("k 0", dict(k=0), "k must be in [1, pool]", None),
           ("k above pool", dict(k=5), "k must be in [1, pool]", None),
           ("lam -0.1", dict(lam=-0.1), "lam must be in [0, 1]", None),
           ("lam NaN", dict(lam=float("nan")), "lam must be in [0, 1]", None),
           ("raw_scores 2", dict(raw=2), "raw_scores must be 0 or 1", None),
           ("null items", dict(items=None), "null outputs", None),
           ("null scores", dict(scores=None), "null outputs", None)]
# the context's own words for the defects the trained calls leave to it
K_CONTEXT = [("k 0", dict(k=0), None, "k must be in [1, 1024]"),
             ("k 1025", dict(k=1025), None, "k must be in [1, 1024]")]
TOP = [("top 0", dict(top=0), None, "top must be in [1, 32]"),
       ("top 33", dict(top=33), None, "top must be in [1, 32]"),
       ("null score", dict(score=None), None, "null pointer")]
SIMILAR = [("null model", dict(model=None), BAD, None),
           ("negative n", dict(n=-1), BAD, None),
           ("null ids", dict(items=None), BAD, None),
           ("unknown flag", dict(sim_flags=4), None, "unknown flag")] + K_CONTEXT

# (entry point, fold-in form, defects)
TABLE = [
    ("recommend", False, trained_rows("recommend") + K_CONTEXT + [
        ("null items", dict(items=None), None, "bad arguments (null outputs)")]),
    ("recommend", True, history_rows() + [
        ("k 0", dict(k=0), K_ITEMS, None), ("k 1025", dict(k=1025), K_ITEMS, None),
        ("null items", dict(items=None), K_ITEMS, None)]),
    ("recommend_diverse", False, trained_rows("recommend_diverse") + DIVERSE),
    ("recommend_diverse", True, history_rows() + DIVERSE),
    ("explain", False, trained_rows("explain") + TOP + [
        ("null tgt_ptr", dict(tgt_ptr=None), BAD, None),
        ("tgt_ptr[0]", dict(tgt_ptr=i64(1, 2, 3)), None, "cand_ptr[0] must be 0"),
        ("target id n_items", dict(tgt_items=i32(2, 0, NI)), None, "candidate id 5 out of range")]),
    ("explain", True, history_rows() + TOP + [("null tgt_ptr", dict(tgt_ptr=None), BAD, None)]),
    ("rank_candidates", False, trained_rows("rank_candidates") + K_CONTEXT + [
        ("null items", dict(items=None), None, "null pointer"),
        ("null cand_ptr", dict(cand_ptr=None), None, "null pointer"),
        ("cand_ptr[0]", dict(cand_ptr=i64(1, 2, 5)), None, "cand_ptr[0] must be 0"),
        ("cand_ptr order", dict(cand_ptr=i64(0, 5, 4)), None, "cand_ptr not monotone at row 1"),
        ("null cand_items", dict(cand_items=None), None, "null cand_items"),
        ("candidate id -1", dict(cand_items=i32(-1, 3, 0, 2, 4)), None,
         "candidate id -1 out of range"),
        ("candidate id n_items", dict(cand_items=i32(1, 3, 0, NI, 4)), None,
         "candidate id 5 out of range")]),
    ("rank_candidates", True, history_rows() + [
        ("k 0", dict(k=0), K_ITEMS, None), ("k 1025", dict(k=1025), K_ITEMS, None),
        ("null items", dict(items=None), K_ITEMS, None),
        ("null cand_ptr", dict(cand_ptr=None), BAD, None),
        ("cand_ptr[0]", dict(cand_ptr=i64(1, 2, 5)), BAD, None),
        ("cand_ptr order", dict(cand_ptr=i64(0, 5, 4)), "cand_ptr not monotone", None),
        ("null cand_items", dict(cand_items=None), "null cand_items", None),
        ("candidate id -1", dict(cand_items=i32(-1, 3, 0, 2, 4)), "candidate id -1 out of range",
         None),
        ("candidate id n_items", dict(cand_items=i32(1, 3, 0, NI, 4)),
         "candidate id 5 out of range", None)]),
    ("evaluate", False, trained_rows("evaluate") + METRICS),
    ("evaluate", True, history_rows() + METRICS),
    ("evaluate_candidates", False, trained_rows("evaluate_candidates") + METRICS + CANDIDATES),
    ("evaluate_candidates", True, history_rows() + METRICS + CANDIDATES),
    ("evaluate_sampled", False, trained_rows("evaluate_sampled") + METRICS + [
        ("negative n_neg", dict(n_neg=-1), "n_neg must not be negative", None)]),
    ("evaluate_sampled", True, history_rows() + METRICS + [
        ("negative n_neg", dict(n_neg=-1), "n_neg must not be negative", None)]),
    ("evaluate_ranks", False, trained_rows("evaluate_ranks") + RANKS),
    ("evaluate_ranks", True, history_rows() + RANKS),
    ("score", False, trained_rows("score") + [
        ("null items", dict(pair_items=None), BAD, None),
        ("null scores", dict(pair_out=None), BAD, None),
        ("item id -1", dict(pair_items=i32(-1, 0)), None, "item id -1 out of range"),
        ("item id n_items", dict(pair_items=i32(4, NI)), None, "item id 5 out of range")]),
    ("similar_items", False, SIMILAR + [
        ("item id -1", dict(sim_rows=i64(0, -1)), None, "row id -1 out of range"),
        ("item id n_items", dict(sim_rows=i64(NI, 0)), None, "row id 5 out of range")]),
    ("similar_users", False, SIMILAR + [
        ("user id -1", dict(users=i64(0, -1)), None, "row id -1 out of range"),
        ("user id n_users", dict(users=i64(NU, 0)), None, "row id 6 out of range")]),
    ("diversify", False, [("null model", dict(model=None), BAD, None),
                          ("negative n", dict(n=-1), BAD, None),
                          ("null lists", dict(lists=None), BAD, None),
                          ("null list_scores", dict(list_scores=None), BAD, None)] + DIVERSE),
]


def message(name, fold, own, ctx):
    return f"{symbol(name, fold)}: {own}" if ctx is None else f"{CONTEXT[name]}: {ctx}"


CASES = [(name, fold, defect, over, message(name, fold, own, ctx))
         for name, fold, defects in TABLE for defect, over, own, ctx in defects]

# Zero rows: (entry point, fold-in form, state, overrides, None = OK or the
# message of FRECSYS_ERR_INVALID, whether `summary` is written or None where
# there is none).
EMPTY = dict(n=0, hist_ptr=i64(0), cand_ptr=i64(0), gt_ptr=i64(0), tgt_ptr=i64(0))
ZERO = ([(name, fold, "valid", EMPTY, None, True if name in EVALS else None)
         for name, fold in ENTRY_POINTS] + [
    ("recommend", False, "k 0", dict(EMPTY, k=0), "recommend: k must be in [1, 1024]", None),
    ("recommend", True, "k 0", dict(EMPTY, k=0), "frecsys_model_recommend_fold_in: " + K_ITEMS,
     None),
    ("evaluate", False, "cut-off 0", dict(EMPTY, k_list=i32(0, 3)),
     "frecsys_model_evaluate: " + CUT_RANGE, False),
    ("evaluate", True, "cut-off 0", dict(EMPTY, k_list=i32(0, 3)),
     "frecsys_model_evaluate_fold_in: " + CUT_RANGE, False),
])


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    trained = fh.Model("ials", TRAIN_USERS, TRAIN_ITEMS, dim=DIM, seed=3)
    trained.initialize()
    trained.train(1)
    path = str(tmp_path_factory.mktemp("model_args") / "tiny.frecsys")
    trained.save(path, include_data=False)
    serve_only = fh.Model.load(path)
    yield {"trained": trained, "serve_only": serve_only}
    serve_only.close()
    trained.close()


def _ids(table):
    return [f"{symbol(t[0], t[1])[14:]}-{t[2]}".replace(" ", "_") for t in table]


def _entry_ids(table):
    return [symbol(name, fold)[14:] for name, fold in table]


@pytest.mark.parametrize("name,fold", ENTRY_POINTS, ids=_entry_ids(ENTRY_POINTS))
def test_defaults_are_valid(models, name, fold):
    # so that each case of CASES has its one defect only; also with the
    # history excluded
    run(models["trained"], name, fold, {})
    run(models["trained"], name, fold, dict(exc=1))


@pytest.mark.parametrize("name,fold,defect,over,msg", CASES, ids=_ids(CASES))
def test_defects(models, name, fold, defect, over, msg):
    with pytest.raises(fh.FrecsysError) as e:
        run(models["trained"], name, fold, over)
    assert e.value.code == INVALID, e.value
    assert str(e.value) == f"frecsys error {INVALID}: {msg}"


@pytest.mark.parametrize("name,fold,state,over,msg,written", ZERO, ids=_ids(ZERO))
def test_zero_rows(models, name, fold, state, over, msg, written):
    if msg is None:
        a = run(models["trained"], name, fold, over)
    else:
        rc, a = call(models["trained"], name, fold, over)
        assert rc == INVALID
        assert models["trained"].lib.frecsys_model_last_error().decode() == msg
    if written is not None:
        # [(2 + 2 na) nk] values, one column for the rank evaluation
        used = (2 + 2 * a["na"]) * (1 if name == "evaluate_ranks" else a["nk"])
        assert np.all(a["summary"][used:] == SENTINEL)
        if written:
            assert np.all(a["summary"][:used] != SENTINEL), a["summary"][:used]
        else:
            assert np.all(a["summary"][:used] == SENTINEL), a["summary"][:used]


SERVE_ONLY = (": the model was loaded without training tuples (serve-only): no training and no "
              "exclude_seen")
# the two list evaluations name themselves together
LISTS = "frecsys_model_evaluate_candidates / _sampled"


def _refused(who, call_it):
    with pytest.raises(fh.FrecsysError) as e:
        call_it()
    assert e.value.code == INVALID, e.value
    assert str(e.value) == f"frecsys error {INVALID}: {who}{SERVE_ONLY}"


def test_serve_only(models):
    m = models["serve_only"]
    for name in PAIRS:
        if name != "explain":  # the others read the tuples only to exclude them
            run(m, name, False, {})
        who = LISTS if name in ("evaluate_candidates", "evaluate_sampled") else symbol(name, False)
        _refused(who, lambda: run(m, name, False, dict(exc=1)))
        run(m, name, True, dict(exc=1))  # the history a fold-in call is given
    for name in SINGLES:
        run(m, name, False, {})
    _refused("frecsys_model_train", m.train)


# three histories where the valid call had two, each with a defect the entry
# point checks itself after the history CSR
THREE = dict(n=3, hist_ptr=i64(0, 1, 3, 4), hist_items=i32(0, 1, 2, 3), gt_ptr=i64(0, 1, 2, 3),
             gt_items=i32(4, 3, 0), cand_ptr=i64(0, 1, 2, 3), cand_items=i32(1, 2, 3),
             tgt_ptr=i64(0, 1, 2, 3), tgt_items=i32(4, 3, 0))
REJECTED = {"recommend": dict(k=0), "recommend_diverse": dict(lam=float("nan")),
            "explain": dict(tgt_ptr=None), "rank_candidates": dict(cand_items=i32(1, NI, 3)),
            "evaluate": dict(k_list=i32(1, 0)), "evaluate_candidates": dict(cand_items=i32(1, -1, 3)),
            "evaluate_sampled": dict(n_neg=-1),
            "evaluate_ranks": dict(rank=None, eligible=None, mrr=None, auc=None, summary=None)}


@pytest.mark.parametrize("name", PAIRS)
def test_checks_come_before_the_projection(models, name):
    m = models["trained"]
    run(m, name, True, {})
    rc, _ = call(m, name, True, dict(THREE, **REJECTED[name]))
    assert rc == INVALID, m.lib.frecsys_model_last_error().decode()
    lengths = m.context().csr_row_lengths(fh.SIDE_EVAL, n=2)
    assert lengths.tolist() == [2, 1], lengths
