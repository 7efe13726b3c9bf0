"""Corpus and classifier of the task-assignment A* (MRP_LL_ASTAR_TA) at the hand-overs between its two tiers and at its
decrease-key branch (tests/test_ta_tier_cases_cpu.py on the CPU, tests/test_ta_tiers_gpu.py on the device).  CPU only: the
engine is never imported.

A case is a dict: name, group, map (dimx, dimy, obstacles), start, goal (None: no task), vc ([t, x, y]), ec
([t, x1, y1, x2, y2]), cap (max_expansions, -1: none) and cfg — the tier limits the case is meant for, as a caller states
them (0 = the engine's default): lds_nodes / lds_rows / lds_path_bytes of mrp_ll_configure_tiers, arena_nodes of
mrp_ll_options.  classify() adds ref (oracle.ta_ll_search with its counters: the reference's answer and what its search
did), cls ("tier": the LDS tier finishes the search, result.tier == 0; "handed_over": the arena tier runs it, result.tier
== 1), why (the one rule that decides, the first that holds in the order below) and emulable.  There is no third class.

The rule (include/mrp_ll.h: MRP_LL_ASTAR_TA, mrp_ll_configure_tiers; csrc/ll_ta.h runJobTA, csrc/ll_compact.h
compactSearchTA), applied to the reference's trajectory:
  shape     a map side above 32, or more than 64 vertex or more than 64 edge constraints (counted as the packer does,
            host/ll_pack.h: entries inside the grid with 0 <= t < max_horizon, duplicates included)
  off       the tier is off: lds_nodes < 0, lds_path_bytes < 2048, or arena_nodes (rounded down to even) < 4096 — the
            64 KiB cameFrom table of the tier does not fit the arena slot's node area
  h_start   the start's table value is above 254 (checked before the first pop, so an expansion cap does not matter)
  open      a node that does not end the search is about to be expanded with open + 5 > open cap, the popped node
            counted.  open cap = min(L / 2, 1023) with L = max(8, min(lds_nodes, 2048) & ~3): the engine rounds
            lds_nodes DOWN to a multiple of 4, so the open cap is always even below 1023
  time      such a node has time > min(lds_rows - 2, 61), lds_rows clamped to 8 .. 64
  field     a newly generated node has h or f above 254
  fits      none of them
At every pop the expansion cap comes first, then the solution test, then open, then time (compactSearchTA): the node that
trips the cap, or is the solution, is "a node that ends the search" and the limits are not applied to it — which is
exactly how oracle/ta_restated.hpp's Counters count.  (The tier also leaves on g > 127; g <= time <= 62 inside it, so
that can never decide, and classify() asserts it.)"""
import json
import os
import sys
from collections import deque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

INT_MAX = 2 ** 31 - 1
# ---- the constants of the engine the classes rest on, named once ----
SIDE = 32            # compactOk: J.dimx <= 32 && J.dimy <= 32
KEYS = 64            # one constraint key per lane
OPEN_MAX = 1023      # ct::kCap: 4 groups of 256 entries, less one
OPEN_ROOM = 5        # nOpen + 5 > openCap: the five successors of one expansion
T_MAX = 61           # ct::kMaxT = kGMax - 2
F_MAX = 254          # the 8-bit f field, 255 - f with 255 left to "no element"
LDS_NODES_MAX = 2048  # kLdsMaxNodes
PATH_BYTES_MIN = 2048
ARENA_NODES_MIN = 4096  # arena_nodes * 16 >= ct::kParentBytes = 64 rows * 1024 cells
MAX_HORIZON = 512
DEFAULT_CFG = dict(lds_nodes=0, lds_rows=0, lds_path_bytes=0, arena_nodes=0)
FIXTURE = os.path.join(ROOT, "tests", "golden", "ta_decrease_key_cases.json")
PATH_CAP = 1024


def bfs_table(dimx, dimy, obstacles, goal):
    """shortest_path_heuristic.hpp's row for `goal`: dist[y][x], INT_MAX = unreachable (what a caller uploads)."""
    obst = {(o[0], o[1]) for o in obstacles}
    dist = [[INT_MAX] * dimx for _ in range(dimy)]
    if tuple(goal) in obst:
        return dist
    dist[goal[1]][goal[0]] = 0
    q = deque([tuple(goal)])
    while q:
        x, y = q.popleft()
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            nx, ny = x + dx, y + dy
            if 0 <= nx < dimx and 0 <= ny < dimy and (nx, ny) not in obst and dist[ny][nx] == INT_MAX:
                dist[ny][nx] = dist[y][x] + 1
                q.append((nx, ny))
    return dist


# ---- the limits an engine applies, from what its caller asked for ----
def open_cap(cfg):
    n = cfg.get("lds_nodes", 0)
    eff = LDS_NODES_MAX if n == 0 else max(8, min(n, LDS_NODES_MAX) & ~3)
    return min(eff // 2, OPEN_MAX)


def max_t(cfg):
    r = cfg.get("lds_rows", 0)
    rows = 64 if r <= 0 else min(max(r, 8), 64)
    return min(rows - 2, T_MAX)


def tier_off(cfg):
    if cfg.get("lds_nodes", 0) < 0:
        return True
    pb = cfg.get("lds_path_bytes", 0)
    if pb > 0 and (min(pb, 65536) & ~31) < PATH_BYTES_MIN:
        return True
    an = cfg.get("arena_nodes", 0)
    return an > 0 and (an & ~1) < ARENA_NODES_MIN


def packed_keys(case):
    """(vertex, edge) constraint words the packer makes of the case's lists."""
    dimx, dimy = case["map"]["dimx"], case["map"]["dimy"]
    nv = sum(1 for t, x, y in case["vc"] if 0 <= t < MAX_HORIZON and 0 <= x < dimx and 0 <= y < dimy)
    ne = sum(1 for t, x1, y1, x2, y2 in case["ec"]
             if 0 <= t < MAX_HORIZON and 0 <= x1 < dimx and 0 <= y1 < dimy and abs(x2 - x1) + abs(y2 - y1) <= 1)
    return nv, ne


def rule(case, ref, cfg):
    """(cls, why) of `case` on an engine configured by `cfg`, from the reference's counters `ref`."""
    nv, ne = packed_keys(case)
    if case["map"]["dimx"] > SIDE or case["map"]["dimy"] > SIDE or nv > KEYS or ne > KEYS:
        return "handed_over", "shape"
    if tier_off(cfg):
        return "handed_over", "off"
    if ref["h_start"] > F_MAX:
        return "handed_over", "h_start"
    if ref["max_open_at_pop"] + OPEN_ROOM > open_cap(cfg):
        return "handed_over", "open"
    if ref["max_time_expanded"] > max_t(cfg):
        return "handed_over", "time"
    if ref["max_h_generated"] > F_MAX or ref["max_f_generated"] > F_MAX:
        return "handed_over", "field"
    return "tier", "fits"


def emulable(case, cfg):
    """compactSearchTA can be asked at all (tests/support/emu_ll.cpp): the shape fits and the tier is on."""
    nv, ne = packed_keys(case)
    return case["map"]["dimx"] <= SIDE and case["map"]["dimy"] <= SIDE and nv <= KEYS and ne <= KEYS and not tier_off(cfg)


def reference(oracle_mod, case):
    return oracle_mod.ta_ll_search(case["map"], case["start"], case["goal"], case["vc"], case["ec"],
                                   cap_expansions=case["cap"], cap=PATH_CAP, counters=True)


def classify(oracle_mod, case):
    ref = reference(oracle_mod, case)
    assert ref["rc"] == -1 or ref["success"], ("the reference never returns from a search without a solution", case["name"])
    case["ref"] = ref
    case["cls"], case["why"] = rule(case, ref, case["cfg"])
    case["emulable"] = emulable(case, case["cfg"])
    if case["cls"] == "tier":
        assert ref["max_time_expanded"] + 1 <= 127  # g <= time: the tier's 7-bit g field never decides
    return case


# ---- the corpus ----
def _case(name, group, m, start, goal, vc=(), ec=(), cap=-1, **cfg):
    c = dict(DEFAULT_CFG)
    c.update(cfg)
    return dict(name=name, group=group, map=m, start=list(start), goal=None if goal is None else list(goal),
                vc=[list(v) for v in vc], ec=[list(e) for e in ec], cap=cap, cfg=c)


EMPTY32 = dict(dimx=32, dimy=32, obstacles=[])


def time_cases():
    """The 6-bit time field: a node at time 62 is never expanded in the tier, so a path whose LAST state has time 62 still
    finishes there (its end is popped, not expanded)."""
    out = []
    for d in range(56, 63):          # corner start, goal d steps away, w forced Waits at the start
        for w in range(4):
            vc = [[t, x, y] for t in range(1, w + 1) for x, y in ((1, 0), (0, 1))]
            out.append(_case("time_corner_d%d_w%d" % (d, w), "time", EMPTY32, (0, 0), (31, d - 31), vc))
    for T in range(58, 66):
        out.append(_case("time_goal_T%d" % T, "time", EMPTY32, (5, 5), (7, 5), [[T, 7, 5]]))
        out.append(_case("time_notask_T%d" % T, "time", EMPTY32, (5, 5), None, [[T, 5, 5]]))
    return out


def rows_variants(classified):
    """Every time case the default tier finishes, under lds_rows = E + 2 (still finished) and E + 1 (handed over), E the
    largest time it expands.  Only the tier flips."""
    out = []
    for c in classified:
        E = c["ref"]["max_time_expanded"]
        if c["group"] != "time" or c["cls"] != "tier" or E + 1 < 8:
            continue
        for rows in (E + 2, E + 1):
            out.append(_case("%s_rows%d" % (c["name"], rows), "rows", c["map"], c["start"], c["goal"], c["vc"], c["ec"],
                             lds_rows=rows))
    return out


# goal-constraint floods on the empty map from (0, 0): goal, time of its constraint.  The first five are the family as the
# issue states it; the next two are the closest pair on either side of 1023 - 5 that scripts/hunt_ta_decrease_keys.py
# --floods finds among goals (a, b) with 10 <= a <= b <= 24 and T = 52 .. 61; the last three have an ODD max_open_at_pop,
# so that open caps of exactly M + 5 and M + 4 can be asked for (the engine keeps lds_nodes / 2 even)
FLOODS = [((14, 14), 60), ((16, 16), 60), ((17, 17), 60), ((18, 18), 60), ((20, 20), 59)]
FLOODS_NEAR = [((19, 19), 57), ((16, 23), 56)]   # max_open_at_pop 1018 and 1020
FLOODS_ODD = [((11, 12), 52), ((11, 15), 59), ((12, 24), 59)]  # 481, 575, 823


def open_cases():
    out = []
    for (gx, gy), T in FLOODS + FLOODS_NEAR + FLOODS_ODD:
        out.append(_case("open_flood_%d_%d_T%d" % (gx, gy, T), "open", EMPTY32, (0, 0), (gx, gy), [[T, gx, gy]]))
    return out


def open_variants(classified):
    """Three floods under an open cap of exactly M + 5 (finished in the tier) and M + 4 (handed over), M = max_open_at_pop."""
    out = []
    names = {"open_flood_%d_%d_T%d" % (g[0], g[1], T) for g, T in FLOODS_ODD}
    for c in classified:
        if c["name"] not in names:
            continue
        M = c["ref"]["max_open_at_pop"]
        assert M % 2 == 1 and M + 5 < OPEN_MAX
        for cap in (M + 5, M + 4):
            out.append(_case("%s_cap%d" % (c["name"], cap), "open_cap", c["map"], c["start"], c["goal"], c["vc"], c["ec"],
                             lds_nodes=2 * cap))
    return out


def constraint_cases():
    """One key per lane: 63, 64 and 65 constraints of a kind on a one-row corridor, the LAST listed the only one that
    matters (cost 6 with it, 5 without); the others lie far away in space and time."""
    m = dict(dimx=32, dimy=1, obstacles=[])
    fill_v = [[100 + i, 12 + i % 20, 0] for i in range(64)]
    fill_e = [[100 + i, 12 + i % 19, 0, 13 + i % 19, 0] for i in range(64)]
    key_v, key_e = [3, 3, 0], [2, 2, 0, 3, 0]
    out = []
    for n in (63, 64, 65):
        out.append(_case("keys_vertex_%d" % n, "constraints", m, (0, 0), (5, 0), fill_v[:n - 1] + [key_v]))
        out.append(_case("keys_edge_%d" % n, "constraints", m, (0, 0), (5, 0), [], fill_e[:n - 1] + [key_e]))
    out.append(_case("keys_vertex_64_edge_64", "constraints", m, (0, 0), (5, 0), fill_v[:63] + [key_v], fill_e[:63] + [key_e]))
    out.append(_case("keys_vertex_64_edge_65", "constraints", m, (0, 0), (5, 0), fill_v[:63] + [key_v], fill_e[:64] + [key_e]))
    return out


def snake_map():
    """32 x 32 with walls on the odd rows 1 .. 21, open at alternating ends: a serpentine whose table values pass 300."""
    obst = [[x, y] for y in range(1, 22, 2) for x in range(32) if x != (31 if (y // 2) % 2 == 0 else 0)]
    return dict(dimx=32, dimy=32, obstacles=obst)


SNAKE_GOAL = (0, 0)
SNAKE_H = (252, 253, 254, 255, 256, 300)


def field_cases():
    """The 8-bit f field: starts on the serpentine whose table value is 252 .. 256 and 300, uncapped (a path beyond 61
    steps: the arena tier in any case) and under an expansion cap of 10 (the class is what the rule gives: h = 252 stays,
    its largest f is 254)."""
    m = snake_map()
    tab = bfs_table(32, 32, m["obstacles"], SNAKE_GOAL)
    out = []
    for h in SNAKE_H:
        # a cell in the middle of a corridor row (both neighbours free), so that a step away from the goal exists
        s = next((x, y) for y in range(32) for x in range(1, 31) if tab[y][x] == h and y % 2 == 0 and y <= 22)
        out.append(_case("field_h%d" % h, "field", m, s, SNAKE_GOAL))
        out.append(_case("field_h%d_cap10" % h, "field", m, s, SNAKE_GOAL, cap=10))
    return out


def side_cases():
    vc, ec = [[4, 7, 3], [9, 12, 5]], [[0, 3, 3, 4, 3]]
    return [_case("side_%dx%d" % (dx, dy), "side", dict(dimx=dx, dimy=dy, obstacles=[[10, 4], [10, 5], [10, 6]]),
                  (3, 3), (20, 9), vc, ec) for dx, dy in ((32, 32), (33, 32), (32, 33))]


def decrease_key_cases():
    """Searches with decrease_keys > 0: the inputs scripts/hunt_ta_decrease_keys.py kept (tests/golden); the oracle and its
    counters are recomputed here."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    return [_case(c["name"], "decrease_key", dict(dimx=c["dimx"], dimy=c["dimy"], obstacles=c["obstacles"]), c["start"],
                  c["goal"], c["vc"], c["ec"]) for c in fx["cases"]]


_CORPUS = None


def corpus(oracle_mod):
    """Every case, classified.  Built once per process and shared: nothing may change it."""
    global _CORPUS
    if _CORPUS is None:
        base = [classify(oracle_mod, c) for c in
                time_cases() + open_cases() + constraint_cases() + field_cases() + side_cases() + decrease_key_cases()]
        more = [classify(oracle_mod, c) for c in rows_variants(base) + open_variants(base)]
        _CORPUS = base + more
        names = [c["name"] for c in _CORPUS]
        assert len(set(names)) == len(names)
    return _CORPUS


def with_cfg(case, **cfg):
    """The class of `case` on an engine with other limits: (cls, why).  The case itself is left as it is."""
    c = dict(case["cfg"])
    c.update(cfg)
    return rule(case, case["ref"], c)
