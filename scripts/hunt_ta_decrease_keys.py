#!/usr/bin/env python3
"""Offline hunt for the inputs of tests/ta_tier_cases.py (CPU only, the oracle and its counters — oracle.ta_ll_search
counters=True):

  python scripts/hunt_ta_decrease_keys.py [--budget N] [--write]
      searches of the task-assignment A* with decrease_keys > 0, N searches (default 4000) from each of five seeded families:
        uniform   random maps 4 x 4 .. 32 x 32, random constraints with times up to 40, a few next to the start
        directed  random 6 x 6 .. 16 x 16 maps with a task, 10 - 50 random vertex constraints with times up to 60, one to
                  three goal constraints in the second half of that range, up to ten constraints around the goal
        near / mid / wide   goalside(): goal constraints and constraints within two steps of the goal, on 4 x 4 .. 7 x 7
                  maps with times below 30, 6 x 6 .. 12 x 12 below 56, 14 x 14 .. 32 x 32 below 60 (the open lists beyond
                  512 entries)
      prints the rates and the largest open size at an event, and with --write keeps a selection (inputs only) in
      tests/golden/ta_decrease_key_cases.json.
      --deep N --probe-lib LIB: N more searches of the wide family, looking for a rediscovered state whose open entry lies
      in the FOURTH 256-entry scan group of compactSearchTA.  The oracle cannot see positions, so the candidates (event
      beyond 768 open entries, finished in the LDS tier, at most 2800 expansions) go through LIB: tests/support/emu_ll.cpp
      built from a scratch copy of csrc/ll_compact.h whose rediscovery scan stops after three groups.  A candidate whose
      result then differs from the oracle's has its entry in the fourth group and is kept (dk_deep_*).
  python scripts/hunt_ta_decrease_keys.py --floods
      the goal-constraint floods on the empty 32 x 32 map: max_open_at_pop next to 1023 - 5 and with odd values.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle  # noqa: E402
import ta_tier_cases as tc  # noqa: E402

MAX_EXPANSIONS = 1500  # what a kept case may cost ...
MAX_EXPANSIONS_DEEP = 2000  # ... unless its event lies beyond 768 open entries: those are rare
MAX_EXPANSIONS_PROBED = 2800  # ... or it is shown to rediscover a state in the fourth scan group (--deep): rarer still


def random_map(rng, lo, hi, density):
    dimx, dimy = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
    n = int(dimx * dimy * density)
    obst = sorted({(int(rng.integers(0, dimx)), int(rng.integers(0, dimy))) for _ in range(n)})
    return dict(dimx=dimx, dimy=dimy, obstacles=[list(o) for o in obst])


def pick_pair(rng, m):
    """A start and a task in one free component (the reference never returns from a search for an unreachable task)."""
    obst = {tuple(o) for o in m["obstacles"]}
    free = [(x, y) for y in range(m["dimy"]) for x in range(m["dimx"]) if (x, y) not in obst]
    if len(free) < 2:
        return None
    s = free[int(rng.integers(0, len(free)))]
    tab = tc.bfs_table(m["dimx"], m["dimy"], m["obstacles"], s)
    reach = [c for c in free if c != s and tab[c[1]][c[0]] < tc.INT_MAX]
    if not reach:
        return None
    return list(s), list(reach[int(rng.integers(0, len(reach)))])


def around(rng, m, cell, n, t_hi):
    out = []
    for _ in range(n):
        dx, dy = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1)][int(rng.integers(0, 7))]
        x, y = cell[0] + dx, cell[1] + dy
        if 0 <= x < m["dimx"] and 0 <= y < m["dimy"]:
            out.append([int(rng.integers(1, t_hi)), x, y])
    return out


def uniform(rng):
    m = random_map(rng, 4, 32, float(rng.uniform(0.0, 0.25)))
    p = pick_pair(rng, m)
    if p is None:
        return None
    s, g = p
    goal = g if rng.integers(0, 2) else None
    vc = [[int(rng.integers(0, 40)), int(rng.integers(0, m["dimx"])), int(rng.integers(0, m["dimy"]))]
          for _ in range(int(rng.integers(0, 50)))]
    vc += around(rng, m, s, int(rng.integers(0, 5)), 12)
    ec = []
    for _ in range(int(rng.integers(0, 20))):
        x, y = int(rng.integers(0, m["dimx"])), int(rng.integers(0, m["dimy"]))
        dx, dy = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)][int(rng.integers(0, 5))]
        ec.append([int(rng.integers(0, 40)), x, y, x + dx, y + dy])
    return m, s, goal, vc, ec


def directed(rng, lo=6, hi=16, density=0.2):
    m = random_map(rng, lo, hi, float(rng.uniform(0.0, density)))
    p = pick_pair(rng, m)
    if p is None:
        return None
    s, g = p
    vc = [[int(rng.integers(0, 60)), int(rng.integers(0, m["dimx"])), int(rng.integers(0, m["dimy"]))]
          for _ in range(int(rng.integers(10, 51)))]
    vc += [[int(rng.integers(30, 60)), g[0], g[1]] for _ in range(int(rng.integers(1, 4)))]
    vc += around(rng, m, g, int(rng.integers(0, 11)), 60)
    uniq = []
    for v in vc:  # distinct, 64 at most: every case is a job of the LDS tier by its shape
        if v not in uniq and v != [0] + s:
            uniq.append(v)
    return m, s, g, uniq[-64:], []


def goalside(rng, lo, hi, t_hi):
    """Two to eight goal constraints and 5 - 40 constraints on the cells within two steps of the goal, times below t_hi:
    the agent is driven off its task and back again and again, each time with another count of free Waits behind it."""
    m = random_map(rng, lo, hi, float(rng.uniform(0.0, 0.15)))
    p = pick_pair(rng, m)
    if p is None:
        return None
    s, g = p
    vc = [[int(rng.integers(3, t_hi)), g[0], g[1]] for _ in range(int(rng.integers(2, 9)))]
    ring = [(g[0] + dx, g[1] + dy) for dx in range(-2, 3) for dy in range(-2, 3) if 0 < abs(dx) + abs(dy) <= 2]
    ring = [c for c in ring if 0 <= c[0] < m["dimx"] and 0 <= c[1] < m["dimy"]]
    for _ in range(int(rng.integers(5, 40))):
        c = ring[int(rng.integers(0, len(ring)))]
        vc.append([int(rng.integers(1, t_hi)), c[0], c[1]])
    uniq = []
    for v in vc:
        if v not in uniq and v != [0] + s:
            uniq.append(v)
    return m, s, g, uniq[-64:], []


FAMILIES = (("uniform", uniform, 101), ("directed", directed, 202),
            ("near", lambda rng: goalside(rng, 4, 7, 30), 303), ("mid", lambda rng: goalside(rng, 6, 12, 56), 404),
            ("wide", lambda rng: goalside(rng, 14, 32, 60), 505))


def hunt(family, n, seed):
    rng = np.random.default_rng(seed)
    found, ran = [], 0
    for _ in range(n):
        job = family(rng)
        if job is None:
            continue
        m, s, g, vc, ec = job
        r = oracle.ta_ll_search(m, s, g, vc, ec, cap_expansions=4 * MAX_EXPANSIONS, cap=tc.PATH_CAP, counters=True)
        ran += 1
        if r["rc"] == 0 and r["success"] and r["decrease_keys"] > 0:
            found.append((r, dict(dimx=m["dimx"], dimy=m["dimy"], obstacles=m["obstacles"], start=s, goal=g, vc=vc, ec=ec)))
    return ran, found


def report(name, ran, found):
    opens = sorted(r["open_at_decrease_key_max"] for r, _ in found)
    print("%-8s %5d searches, %3d with a decrease-key event (%.2f %%); open size at an event: max %s, > 256: %d, > 512: %d, "
          "> 768: %d; two or more events: %d; re-parented state on the path: %d; beyond time 61: %d" % (
              name, ran, len(found), 100.0 * len(found) / max(ran, 1), opens[-1] if opens else "-",
              sum(o > 256 for o in opens), sum(o > 512 for o in opens), sum(o > 768 for o in opens),
              sum(r["decrease_keys"] >= 2 for r, _ in found), sum(r["reparented_on_path"] > 0 for r, _ in found),
              sum(r["max_time_expanded"] > 61 for r, _ in found)))


def floods():
    m = tc.EMPTY32
    rows = []
    for a in range(10, 25):
        for b in range(a, 25):
            for T in range(52, 62):
                r = oracle.ta_ll_search(m, [0, 0], [a, b], [[T, a, b]], cap_expansions=3000, counters=True)
                if r["rc"] == 0:
                    rows.append((r["max_open_at_pop"], r["expanded"], a, b, T))
    edge = tc.OPEN_MAX - tc.OPEN_ROOM
    below = max(x for x in rows if x[0] <= edge)
    above = min(x for x in rows if x[0] > edge)
    print("closest to %d: below %s, above %s  (max_open_at_pop, expanded, gx, gy, T)" % (edge, below, above))
    odd = sorted(x for x in rows if x[0] % 2 == 1 and x[1] <= MAX_EXPANSIONS)
    print("odd max_open_at_pop: %d of %d; smallest, middle, largest below the edge: %s %s %s" % (
        len(odd), len(rows), odd[0] if odd else None, odd[len(odd) // 2] if odd else None,
        max((x for x in odd if x[0] <= edge), default=None)))


def deep(budget, probe_lib):
    import ctypes
    from test_compact_emu import emu_search_ta
    L = ctypes.CDLL(os.path.abspath(probe_lib))
    ran, found = hunt(FAMILIES[4][1], budget, FAMILIES[4][2])
    cand = [(r, c) for r, c in found if r["open_at_decrease_key_max"] > 768 and r["expanded"] <= MAX_EXPANSIONS_PROBED and
            r["max_open_at_pop"] + tc.OPEN_ROOM <= tc.OPEN_MAX and r["max_time_expanded"] <= tc.T_MAX]
    hits = []
    for r, c in cand:
        e = emu_search_ta(L, dict(dimx=c["dimx"], dimy=c["dimy"], obstacles=c["obstacles"]), c["start"], c["goal"], c["vc"], c["ec"])
        if (e["status"], e["expanded"], e["states"]) != (0, r["expanded"], [s[1:] for s in r["states"]]):
            hits.append(("deep", r, c))
    print("deep     %5d searches, %d candidates beyond 768 open entries in the tier, %d with the entry in the fourth scan group"
          % (ran, len(cand), len(hits)))
    return hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deep", type=int, default=0)
    ap.add_argument("--probe-lib")
    ap.add_argument("--budget", type=int, default=4000)
    ap.add_argument("--floods", action="store_true")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    if a.floods:
        return floods()
    kept = []
    for name, fam, seed in FAMILIES:
        ran, found = hunt(fam, a.budget, seed)
        report(name, ran, found)
        kept += [(name, r, c) for r, c in found if r["expanded"] <= MAX_EXPANSIONS or
                 (r["open_at_decrease_key_max"] > 768 and r["expanded"] <= MAX_EXPANSIONS_DEEP)]
    # the selection: the largest open lists at an event (beyond 768, 512, 256), then the searches with most events, then those with a
    # re-parented state on the returned path, then the cheapest of the rest up to 27 cases
    def take(pred, k, key):
        got = 0
        for item in sorted(kept, key=key):
            if got < k and pred(item[1]) and item not in chosen:
                chosen.append(item)
                got += 1
    chosen = deep(a.deep, a.probe_lib) if a.deep and a.probe_lib else []
    take(lambda r: r["open_at_decrease_key_max"] > 768, 2, lambda it: -it[1]["open_at_decrease_key_max"])
    take(lambda r: r["open_at_decrease_key_max"] > 512, 4, lambda it: -it[1]["open_at_decrease_key_max"])
    take(lambda r: r["open_at_decrease_key_max"] > 256, 5, lambda it: -it[1]["open_at_decrease_key_max"])
    take(lambda r: r["decrease_keys"] >= 2, 5, lambda it: -it[1]["decrease_keys"])
    take(lambda r: r["reparented_on_path"] > 0, 5, lambda it: it[1]["expanded"])
    take(lambda r: True, max(0, 27 - len(chosen)), lambda it: it[1]["expanded"])
    cases = []
    for i, (fam, r, c) in enumerate(chosen):
        c = dict(c, name="dk_%s_%02d" % (fam, i))
        cases.append(c)
        print("  %s: %dx%d, %d events, open %d, expanded %d, on path %d, max time %d" % (
            c["name"], c["dimx"], c["dimy"], r["decrease_keys"], r["open_at_decrease_key_max"], r["expanded"],
            r["reparented_on_path"], r["max_time_expanded"]))
    if a.write:
        with open(tc.FIXTURE, "w") as f:
            json.dump(dict(note="inputs only; made by scripts/hunt_ta_decrease_keys.py --write", cases=cases), f,
                      separators=(",", ":"))
        print("wrote %d cases to %s" % (len(cases), os.path.relpath(tc.FIXTURE, ROOT)))


if __name__ == "__main__":
    main()
