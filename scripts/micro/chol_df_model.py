#!/usr/bin/env python3
"""Discrete-event model of the dataflow Cholesky (csrc/chol.h chol_solve_df)
at T tiles with NW waves: the chain wave runs S(p+1, p), U(p+1, p+1, p),
F(p+1) per panel; with NW >= 8 one further wave runs the forward substitution
and NW - 2 waves are workers, else NW - 1.  Each wave runs its tasks in order,
starting a task when its inputs are final.  Costs are cycles per task (the
measured per-phase profiles of DESIGN.md section 3.1).

Two ways of dealing the worker tasks (S(I, p), I >= p + 2, and every U but
the chain's) are modelled:
  round-robin  task k of the kernel's loop order (panel by panel: TRSMs, then
               the updates column by column) goes to worker k % workers;
  list         a list schedule: the chain stays on wave 0, the earliest-free
               worker takes the task that can start earliest among those whose
               inputs are already scheduled, ties broken by the longest
               remaining path.  The tasks and their costs are the same, only
               the task -> worker assignment and each worker's order change.

Usage:
  chol_df_model.py [chain_factor_cycles worker_task_cycles]
      end time of the chain, its waits and the workers' end time at T = 8,
      NW = 8, round-robin, for the given costs or a grid of them
  chol_df_model.py --compare T,NW [T,NW ...] [--factor F] [--task W]
      the same three numbers under round-robin and under the list schedule
  chol_df_model.py --emit-header T,NW [T,NW ...] [--factor F] [--task W]
      the list schedules' per-worker task lists as a C++ header (stdout);
      csrc/chol_sched.h is this output, committed
"""
import argparse
import sys

CS, CU = 1890, 1000   # chain TRSM / chain update (fused into the factor)
WB = 400              # a worker TRSM's rhs update B(I, p)
CF, WT = 6400, 3600   # measured: chain factor / worker task


def n_workers(NW):
    return NW - 2 if NW >= 8 else NW - 1


def deps(t):
    if t[0] == "F":
        p = t[1]
        return [("U", p, p, p - 1)] if p > 0 else []
    if t[0] == "S":
        i, p = t[1], t[2]
        return [("F", p)] + ([("U", i, p, p - 1)] if p > 0 else [])
    i, j, p = t[1], t[2], t[3]
    return [("S", i, p), ("S", j, p)] + ([("U", i, j, p - 1)] if p > 0 else [])


def chain_tasks(T=8):
    chain = []
    for p in range(-1, T - 1):
        if p >= 0:
            chain += [("S", p + 1, p), ("U", p + 1, p + 1, p)]
        chain.append(("F", p + 1))
    return chain


def worker_tasks(T=8):
    order = []
    for p in range(T - 1):
        order += [("S", i, p) for i in range(p + 2, T)]
        for j in range(p + 1, T):
            order += [("U", i, j, p) for i in range(p + 2 if j == p + 1 else j, T)]
    return order


def round_robin(T=8, NW=8):
    """The kernel's loop-order dealing: per-worker task lists."""
    nwk = n_workers(NW)
    waves = [[] for _ in range(nwk)]
    for k, t in enumerate(worker_tasks(T)):
        waves[k % nwk].append(t)
    return waves


def _costs(cf, wt, nwk):
    return [{"F": cf, "S": CS, "U": CU}] + [{"S": wt + WB, "U": wt}] * nwk


def simulate(cf, wt, T=8, NW=8, waves=None):
    """(chain end, chain waits, workers' end) of per-worker lists `waves`
    (default: round-robin)."""
    if waves is None:
        waves = round_robin(T, NW)
    seqs = [chain_tasks(T)] + waves
    cost = _costs(cf, wt, len(waves))
    done, pos = {}, [0] * len(seqs)
    now, wait = [0.0] * len(seqs), [0.0] * len(seqs)
    progress = True
    while progress:
        progress = False
        for i, seq in enumerate(seqs):
            while pos[i] < len(seq):
                t = seq[pos[i]]
                if not all(d in done for d in deps(t)):
                    break
                start = max([now[i]] + [done[d] for d in deps(t)])
                wait[i] += start - now[i]
                now[i] = start + cost[i][t[0]]
                done[t] = now[i]
                pos[i] += 1
                progress = True
    assert all(pos[i] == len(s) for i, s in enumerate(seqs)), "deadlock"
    return now[0], wait[0], max(now[1:])


def list_schedule(cf, wt, T=8, NW=8):
    """Per-worker task lists of the list schedule (see the module docstring)."""
    nwk = n_workers(NW)
    chain = chain_tasks(T)
    on_chain = set(chain)
    cost = _costs(cf, wt, nwk)
    tcost = {t: cost[0][t[0]] for t in chain}
    tcost.update({t: cost[1][t[0]] for t in worker_tasks(T)})
    # longest path from a task's start to the end of the graph
    succ = {t: [] for t in tcost}
    for t in tcost:
        for d in deps(t):
            succ[d].append(t)
    rem = {}

    def remaining(t):
        if t not in rem:
            rem[t] = tcost[t] + max([remaining(s) for s in succ[t]], default=0)
        return rem[t]

    done, cpos, cnow = {}, 0, 0.0
    free = [0.0] * nwk
    waves = [[] for _ in range(nwk)]
    todo = list(worker_tasks(T))  # loop order: the last tie-break
    while todo or cpos < len(chain):
        while cpos < len(chain) and all(d in done for d in deps(chain[cpos])):
            t = chain[cpos]
            cnow = max([cnow] + [done[d] for d in deps(t)]) + tcost[t]
            done[t] = cnow
            cpos += 1
        ready = [t for t in todo if all(d in done for d in deps(t))]
        if not ready:
            assert cpos == len(chain) and not todo, "the chain waits for an unscheduled task"
            break
        w = min(range(nwk), key=lambda i: free[i])

        def start(t):
            return max([free[w]] + [done[d] for d in deps(t)])

        t = min(ready, key=lambda t: (start(t), -remaining(t)))
        free[w] = start(t) + tcost[t]
        done[t] = free[w]
        waves[w].append(t)
        todo.remove(t)
        assert t not in on_chain
    return waves


def compare(cf, wt, T, NW):
    """{"rr": (chain, waits, workers end), "list": (...)} for one (T, NW)."""
    return {"rr": simulate(cf, wt, T, NW),
            "list": simulate(cf, wt, T, NW, list_schedule(cf, wt, T, NW))}


# a packed task of the header: kind (1 = U) << 12 | I << 8 | J << 4 | p
def pack(t):
    if t[0] == "S":
        return t[1] << 8 | t[2] << 4 | t[2]
    return 1 << 12 | t[1] << 8 | t[2] << 4 | t[3]


END = 0xFFFF  # past a list's end (the kernel reads one entry ahead)


def emit_header(configs, cf, wt, argv):
    out = []
    out.append("// Generated by scripts/micro/chol_df_model.py " + " ".join(argv))
    out.append("// (the output is this file; tests/test_chol_sched_cpu.py regenerates and")
    out.append("// compares it).  Do not edit by hand.")
    out.append("//")
    out.append("// Static worker schedules of the dataflow Cholesky (chol.h chol_solve_df):")
    out.append("// per (T, NW) and worker slot the slot's tasks in the order it runs them,")
    out.append("// from the model's list schedule.  A task is packed as")
    out.append("//   kind << 12 | I << 8 | J << 4 | p     kind 0: S(I, p) with its B(I, p)")
    out.append("//                                        kind 1: U(I, J, p)")
    out.append("// and every list ends in kCholSchedEnd entries up to the common length")
    out.append("// (a worker reads its next entry before it runs the current one).")
    out.append("#pragma once")
    out.append("")
    out.append("namespace frecsys_hip {")
    out.append("")
    out.append(f"constexpr unsigned short kCholSchedEnd = 0x{END:04x};")
    out.append("")
    out.append("// no table: the instantiation keeps the round-robin loops")
    out.append("template <int T, int NW>")
    out.append("struct CholSched {")
    out.append("  static constexpr bool kHas = false;")
    out.append("};")
    for T, NW in configs:
        waves = list_schedule(cf, wt, T, NW)
        c, w, e = simulate(cf, wt, T, NW, waves)
        c0, w0, e0 = simulate(cf, wt, T, NW)
        rr = round_robin(T, NW)
        mx = max(len(s) for s in waves + rr)
        out.append("")
        out.append(f"// T = {T}, NW = {NW} ({len(waves)} workers): model chain {c:.0f}, chain waits {w:.0f},")
        out.append(f"// workers end {e:.0f} (round-robin: {c0:.0f}, {w0:.0f}, {e0:.0f})")
        out.append("template <>")
        out.append(f"struct CholSched<{T}, {NW}> {{")
        out.append("  static constexpr bool kHas = true;")
        out.append(f"  static constexpr int kSlots = {len(waves)}, kMax = {mx};")
        for name, lists in (("", waves), ("Rr", rr)):
            if name:
                out.append("  // the round-robin dealing in loop order (schedule switch off)")
            out.append(f"  static constexpr int k{name}Len[{len(lists)}] = {{" +
                       ", ".join(str(len(s)) for s in lists) + "};")
            out.append(f"  static constexpr unsigned short k{name}Task[{len(lists)}][{mx + 1}] = {{")
            for s in lists:
                words = [pack(t) for t in s] + [END] * (mx + 1 - len(s))
                names = " ".join(f"{t[0]}{''.join(map(str, t[1:]))}" for t in s)
                out.append("      // " + names)
                out.append("      {" + ", ".join(f"0x{x:04x}" for x in words) + "},")
            out.append("  };")
        out.append("};")
    out.append("")
    out.append("}  // namespace frecsys_hip")
    return "\n".join(out) + "\n"


def _config(s):
    t, nw = s.split(",")
    return int(t), int(nw)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("costs", nargs="*", type=float, help="chain_factor_cycles worker_task_cycles")
    ap.add_argument("--compare", nargs="+", type=_config, metavar="T,NW")
    ap.add_argument("--emit-header", nargs="+", type=_config, metavar="T,NW")
    ap.add_argument("--factor", type=float, default=CF)
    ap.add_argument("--task", type=float, default=WT)
    a = ap.parse_args(argv)
    if a.emit_header:
        sys.stdout.write(emit_header(a.emit_header, a.factor, a.task, argv))
        return
    if a.compare:
        for T, NW in a.compare:
            r = compare(a.factor, a.task, T, NW)
            for name in ("rr", "list"):
                c, w, e = r[name]
                print(f"T {T} NW {NW} ({n_workers(NW)} workers)  {name:4s}:  chain {c:7.0f}  "
                      f"chain waits {w:6.0f}  workers end {e:7.0f}")
        return
    if len(a.costs) == 2:
        grid = [(a.costs[0], a.costs[1])]
    elif not a.costs:
        grid = [(cf, wt) for cf in (6800, 5500, 4500) for wt in (3600, 3200, 2800, 2400)]
    else:
        ap.error("give both costs or neither")
    for cf, wt in grid:
        c, w, e = simulate(cf, wt)
        print(f"factor {cf:6.0f}  worker task {wt:6.0f}:  chain {c:7.0f}  "
              f"chain waits {w:6.0f}  workers end {e:7.0f}")


if __name__ == "__main__":
    main()
