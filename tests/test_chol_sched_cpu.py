"""The static worker schedules of the dataflow Cholesky: the generator
(scripts/micro/chol_df_model.py), the committed header it emits
(csrc/chol_sched.h) and the model numbers DESIGN.md section 3.1 quotes.

A schedule is one task list per worker wave.  The kernel's waves run their
lists in order and block on version counters, so a list set is usable exactly
when (a) every worker task is in it once and (b) the data edges together with
every wave's own sequence form an acyclic graph -- then no wave can wait for
something that is behind itself.  (b) is checked on the graph and again by
stepping the kernel's counters through random interleavings.
"""
import importlib.util
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "scripts", "micro", "chol_df_model.py")
HEADER = os.path.join(ROOT, "safer2-recommender_amd", "csrc", "chol_sched.h")

_spec = importlib.util.spec_from_file_location("chol_df_model", GEN)
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

EMITTED = [(8, 8)]
# not emitted, but the generator can produce them: fewer tiles (T = 7 is
# modelled in DESIGN.md and measured without a gain), 4- and 6-wave layouts (no
# wave of its own for the forward substitution), more tiles
OTHERS = [(7, 8), (6, 8), (5, 8), (8, 6), (5, 4), (3, 4), (2, 2), (10, 8)]
QUOTED = [(8, 8), (7, 8)]  # the rows of DESIGN.md's model table
CONFIGS = EMITTED + OTHERS


def _lists(T, NW, which):
    return M.list_schedule(M.CF, M.WT, T, NW) if which == "list" else M.round_robin(T, NW)


def _expected_tasks(T):
    s = {("S", I, p) for p in range(T - 1) for I in range(p + 2, T)}
    u = {("U", I, J, p) for p in range(T - 1) for J in range(p + 1, T) for I in range(J, T)}
    return s | (u - {("U", p + 1, p + 1, p) for p in range(T - 1)})


def _wave_sequences(T, NW, lists):
    """Every wave's tasks in its order, with the rhs tasks the model leaves out:
    a worker's S(I, p) is followed by its B(I, p); Y(p) and B(p+1, p) run on
    the chain (NW < 8) or on a wave of their own."""
    if NW >= 8:
        chain, ywave = [("F", 0)], [("Y", 0)]
        for p in range(T - 1):
            chain += [("S", p + 1, p), ("U", p + 1, p + 1, p), ("F", p + 1)]
            ywave += [("B", p + 1, p), ("Y", p + 1)]
        seqs = [chain, ywave]
    else:
        chain = [("F", 0), ("Y", 0)]
        for p in range(T - 1):
            chain += [("S", p + 1, p), ("B", p + 1, p), ("U", p + 1, p + 1, p), ("F", p + 1),
                      ("Y", p + 1)]
        seqs = [chain]
    for l in lists:
        s = []
        for t in l:
            s.append(t)
            if t[0] == "S":
                s.append(("B", t[1], t[2]))
        seqs.append(s)
    return seqs


def _data_deps(t):
    k = t[0]
    if k == "F":
        p = t[1]
        return [("U", p, p, p - 1)] if p > 0 else []
    if k == "S":
        I, p = t[1], t[2]
        return [("F", p)] + ([("U", I, p, p - 1)] if p > 0 else [])
    if k == "U":
        I, J, p = t[1:]
        return [("S", I, p), ("S", J, p)] + ([("U", I, J, p - 1)] if p > 0 else [])
    if k == "B":
        I, p = t[1], t[2]
        return [("S", I, p), ("Y", p)] + ([("B", I, p - 1)] if p > 0 else [])
    p = t[1]  # Y
    return [("F", p)] + ([("B", p, p - 1)] if p > 0 else [])


@pytest.mark.parametrize("T,NW", CONFIGS)
@pytest.mark.parametrize("which", ["list", "rr"])
def test_every_worker_task_once(T, NW, which):
    lists = _lists(T, NW, which)
    assert len(lists) == M.n_workers(NW)
    flat = [t for l in lists for t in l]
    assert len(flat) == len(set(flat))
    assert set(flat) == _expected_tasks(T)


@pytest.mark.parametrize("T,NW", CONFIGS)
@pytest.mark.parametrize("which", ["list", "rr"])
def test_wait_graph_acyclic(T, NW, which):
    seqs = _wave_sequences(T, NW, _lists(T, NW, which))
    nodes = [t for s in seqs for t in s]
    assert len(nodes) == len(set(nodes))
    pred = {t: list(_data_deps(t)) for t in nodes}
    for s in seqs:
        for a, b in zip(s, s[1:]):
            pred[b].append(a)
    assert all(d in pred for t in nodes for d in pred[t])  # every input is somebody's task
    # Kahn: all nodes leave <=> acyclic
    succ = {t: [] for t in nodes}
    for t in nodes:
        for d in pred[t]:
            succ[d].append(t)
    indeg = {t: len(pred[t]) for t in nodes}
    ready = [t for t in nodes if indeg[t] == 0]
    seen = 0
    while ready:
        t = ready.pop()
        seen += 1
        for s in succ[t]:
            indeg[s] -= 1
            if indeg[s] == 0:
                ready.append(s)
    assert seen == len(nodes), "a cycle: some wave waits for a task behind itself"


def _step(t, ver, bver, yver):
    """The kernel's counters for task t: returns False when a wait is not yet
    satisfied, else checks the counters it overwrites and publishes."""
    k = t[0]
    if k == "F":
        p = t[1]
        if ver.get((p, p), 0) < p:
            return False
        assert ver.get((p, p), 0) == p
        ver[(p, p)] = p + 1
    elif k == "S":
        I, p = t[1], t[2]
        if ver.get((p, p), 0) < p + 1 or ver.get((I, p), 0) < p:
            return False
        assert ver.get((I, p), 0) == p
        ver[(I, p)] = p + 1
    elif k == "U":
        I, J, p = t[1:]
        if ver.get((I, p), 0) < p + 1 or ver.get((J, p), 0) < p + 1 or ver.get((I, J), 0) < p:
            return False
        assert ver.get((I, J), 0) == p  # the updates of a tile land in panel order
        ver[(I, J)] = p + 1
    elif k == "B":
        I, p = t[1], t[2]
        if yver[0] < p + 1 or bver.get(I, 0) < p or ver.get((I, p), 0) < p + 1:
            return False
        assert bver.get(I, 0) == p
        bver[I] = p + 1
    else:
        p = t[1]
        if ver.get((p, p), 0) < p + 1 or bver.get(p, 0) < p:
            return False
        assert yver[0] == p
        yver[0] = p + 1
    return True


@pytest.mark.parametrize("T,NW", CONFIGS)
@pytest.mark.parametrize("which", ["list", "rr"])
def test_random_interleavings_finish(T, NW, which):
    seqs = _wave_sequences(T, NW, _lists(T, NW, which))
    total = sum(len(s) for s in seqs)
    n_runs = 3000 if (T, NW) in QUOTED else 300
    for seed in range(n_runs):
        rng = random.Random(seed)
        ver, bver, yver = {}, {}, [0]
        pos = [0] * len(seqs)
        done = 0
        while done < total:
            order = [w for w in range(len(seqs)) if pos[w] < len(seqs[w])]
            rng.shuffle(order)
            for w in order:  # the first wave, in this run's order, that can advance
                if _step(seqs[w][pos[w]], ver, bver, yver):
                    pos[w] += 1
                    done += 1
                    break
            else:
                raise AssertionError(f"seed {seed}: every wave waits, at {pos}")
        # final versions: a diagonal tile p + 1, L_Ip p + 1, all of b updated
        assert all(ver[(I, J)] == J + 1 for J in range(T) for I in range(J, T))
        assert yver[0] == T and all(bver.get(I, 0) == I for I in range(1, T))


def test_header_is_what_the_generator_emits():
    text = open(HEADER).read()
    first = text.splitlines()[0]
    m = re.match(r"// Generated by scripts/micro/chol_df_model\.py (.*)$", first)
    assert m, first
    argv = m.group(1).split()
    assert argv[0] == "--emit-header"
    configs = [M._config(a) for a in argv[1:] if not a.startswith("-")]
    assert configs == EMITTED and len(configs) == len(argv) - 1  # default costs
    assert M.emit_header(configs, M.CF, M.WT, argv) == text


@pytest.mark.parametrize("T,NW", EMITTED)
def test_header_tables_hold_the_lists(T, NW):
    """The packed words of the committed header decode to the lists."""
    text = open(HEADER).read()
    body = text[text.index(f"struct CholSched<{T}, {NW}>"):]
    body = body[:body.index("};\n", body.index("kRrTask")) + 3]
    for name, which in (("kTask", "list"), ("kRrTask", "rr")):
        lists = _lists(T, NW, which)
        rows = re.findall(r"\{((?:0x[0-9a-f]{4}(?:, )?)+)\}", body[body.index(f" {name}["):])[:len(lists)]
        width = {len(r.split(", ")) for r in rows}
        assert width == {max(len(l) for l in _lists(T, NW, "list") + _lists(T, NW, "rr")) + 1}
        for row, l in zip(rows, lists):
            words = [int(x, 16) for x in row.split(", ")]
            dec = [("U", w >> 8 & 15, w >> 4 & 15, w & 15) if w >> 12 else ("S", w >> 8 & 15, w & 15)
                   for w in words[:len(l)]]
            assert dec == l
            assert all(w == M.END for w in words[len(l):]) and len(words) > len(l)


def _k(x):
    return f"{int(x / 100 + 0.5) / 10:.1f}K"  # to 0.1K, halves up


def test_design_quotes_the_model_numbers():
    """DESIGN.md 3.1 quotes chain / chain waits of both dealings at T = 8 and
    T = 7 as 'chain / waits' in K cycles: they are what the model gives now."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 3.1 "):design.index("### 3.2 ")]
    for T, NW in QUOTED:
        r = M.compare(M.CF, M.WT, T, NW)
        assert r["list"][0] < r["rr"][0] and r["list"][1] < r["rr"][1]
        for name in ("rr", "list"):
            c, w, _ = r[name]
            quote = f"{_k(c)} / {_k(w)}"
            assert quote in sec, (T, NW, name, quote)
    # T <= 6: nothing to gain in the model (the chain hardly waits)
    for T, NW in [(6, 8), (5, 8), (4, 4)]:
        r = M.compare(M.CF, M.WT, T, NW)
        assert r["list"][0] == r["rr"][0]
