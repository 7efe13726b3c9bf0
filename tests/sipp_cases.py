"""Corpus and classifier of the SIPP limit tests (tests/test_sipp_cases_cpu.py on the CPU, tests/test_sipp_limits_gpu.py on
the device): MRP_LL_SIPP on non-square maps, at the hand-overs between its memory tiers, on the table shapes the random
generators of the parity tests never make, and at the limits include/mrp_ll.h documents for it.  CPU only: the engine is
never imported.

A case is a dict: name, group, engine (a key of ENGINES), form, map, start, goal, t0 (SIPP::search's startTime),
intervals ([x, y, s, e] collision intervals), pre (resident only: the first `pre` entries of intervals are added before a
warm-up job on the table, the rest after it, so the job under test carries them as a DELTA; None: one fresh table).
The forms:
  job       the collision_* arrays of mrp_ll_job, batch mode.  Consecutive entries of one location form one list; a
            location given twice keeps the later list (example/sipp.cpp:196-205 calls setCollisionIntervals per entry).
  table     an mrp_ll_sipp_table, batch mode: the table travels whole.  Every entry is one mrp_ll_sipp_table_add, in order.
  resident  the same table inside mrp_ll_session_begin_sipp: the device-resident copy (unless it does not fit the resident
            layout: more than 15 safe intervals on a cell, or a finite bound >= 65535 — then it travels whole).

classify() adds ref (oracle.sipp_single_counted: the reference's answer and its counters), K and S (listed cells and safe
intervals on them), travels, cls, expect, tier and why.  Every class follows from the reference's counters alone; the
limits are the ones include/mrp_ll.h states for MRP_LL_SIPP (csrc/ll_sipp.h is where they are enforced):

  start time  t0 > G_MAX                                                        -> BAD_JOB      (packSipp*, host/ll_pack.h)
  table       a travelling table with 4 * ((cells + 1) / 2 + K + 1 + 2 * S) > TABLE_BYTES or
              cells + S > max_horizon * ((max_cells + 31) / 32)                 -> CAP_NODES    (runSipp, before the search)
  arrival     the largest arrival time of any neighbour getNeighbors emitted (closed ones included: the kernel tests the
              candidates before it looks at their status) > G_MAX               -> CAP_HORIZON  (lateMask / t > kGMask)
  path        2 * raw A* states > max_horizon                                   -> CAP_HORIZON  (len * 2 > out_stride)
  nodes       created (start + first discoveries) > arena_nodes                 -> CAP_NODES
  inside      none of them: the engine equals the reference bit for bit.
  outside     exactly one of them (asserted; a case beyond two would not say which branch answered).
There is no class that allows two answers.  (The kernel also ends a job that EXPANDS a node of g = 1023 which is not the
goal; such a node has f >= 1024, so no search that succeeds with cost <= 1023 expands one, and classify() asserts that an
inside case without a solution never generated an arrival of 1023.)

The tier a resident job must report (result.tier; runSipp, ll_sipp.h) follows from the trajectory (nodes created, open-list
size) at the start of every expansion, the goal's included:
  0   TierLdsSipp to the end
  2   handed over to TierMix at the first expansion with nodes + ROOM > LDS_NODES - 1 or open + ROOM > LDS_NODES
  3   handed over again, at that expansion or a later one, with open + ROOM > MIX_OPEN (or nodes + ROOM > arena_nodes)
  1   every job whose table travels, and a resident job that ends before the search (no safe interval at t0).
open <= nodes, so the open condition of the first hand-over (open > 708) implies the node condition (nodes > 707): it can
never fire alone, and no search can come within 8 entries of it from below without having left the tier (708 - 8 open
entries need 700 nodes from at most 6 pops; an expansion creates at most 60).  The cases on both sides of a hand-over are
therefore placed at the node condition of the first and at the open condition of the second; classify() asserts the
implication.  They come from a comb: a corridor whose every cell has a side cell with m late safe intervals (arrival 900:
never expanded), so an expansion adds m + 1 nodes and m open entries and the goal's block time T sets the number of
expansions — the trajectory moves in steps of at most 8."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import limit_cases as lc  # noqa: E402

INT_MAX = 2 ** 31 - 1
# ---- the constants of the engine the classes rest on, named once (csrc/ll_sipp.h, csrc/ll_device.h, csrc/host/ll_pack.h) ----
G_MAX = 1023            # kGMask: the 10-bit g field of every open key
LDS_NODES = 768         # MRP_LL_SIPP_LDS_NODES = kSippLdsCap: node records (ids 0 .. 766) and 32-bit open entries of TierLdsSipp
MIX_OPEN = 1152         # (kSippLdsBytes - 16) / 8: 64-bit open entries of TierMix
ROOM = 60               # 4 * kSippCap: free records / entries sippLoop wants before an expansion in an LDS tier
SIPP_CAP = 15           # kSippCap: safe intervals per cell of the resident layout
END_INF = 65535         # kSippEndInf: finite bounds of the resident layout are below it
TABLE_BYTES = 128 * 1024  # arenaPathsBytes: the slot area a travelling table is copied into
NEAR = 8                # "next to a hand-over": within this many nodes / entries
TRAJ_CAP = 400_000
PATH_CAP = 2048

# the option sets (mrp_ll_options) of the engines the device test creates
ENGINES = {
    # 255 x 255 only: a resident table of this engine takes 8 MB whatever its map
    "big": dict(slots=32, n_tickets=1, arena_nodes=131072, max_horizon=512, max_cells=65025, lds_nodes=0),
    "std": dict(slots=32, n_tickets=1, arena_nodes=131072, max_horizon=512, max_cells=4096, lds_nodes=0),
    "long": dict(slots=32, n_tickets=1, arena_nodes=131072, max_horizon=1024, max_cells=4096, lds_nodes=0),
    "small": dict(slots=32, n_tickets=1, arena_nodes=4096, max_horizon=512, max_cells=4096, lds_nodes=-1),
    # max_cells = the map's: the status-word condition of the travelling-table limit binds before the byte condition
    "tiny": dict(slots=32, n_tickets=1, arena_nodes=131072, max_horizon=512, max_cells=64, lds_nodes=0),
}
FORMS = ("job", "table", "resident")
GEOMETRY_DIMS = ((33, 31), (31, 33), (100, 37), (37, 100), (7, 5), (3, 255), (255, 3), (255, 1), (1, 255), (255, 255), (1, 1))
RESIDENT_LISTS = (1, 3, 4, 5, 7, 8, 9, 14, 15)     # record sizes 4, 4, 4, 8, 8, 8, 16, 16, 16 bounds words
LONG_LISTS = (16, 17, 40, 64, 65, 130)             # the cMax > 16 branch: one, two (65) and three (130) passes of 64


def safe_from(collisions):
    """SIPPEnvironment::setCollisionIntervals (sipp.hpp:245-284) for one non-empty list."""
    out, start, last_end = [], 0, 0
    for s, e in sorted(collisions, key=lambda v: v[0]):
        if start <= s - 1:
            out.append([start, s - 1])
        start, last_end = e + 1, e
    if last_end < INT_MAX:
        out.append([start, INT_MAX])
    return out


def cell_lists(case):
    """{(x, y): collision list} as the form hands it to setCollisionIntervals (module docstring); in-grid cells only."""
    m, lists = case["map"], {}
    prev = None
    for x, y, s, e in case["intervals"]:
        c = (x, y)
        if case["form"] == "job" and c != prev:
            lists.pop(c, None)   # a new entry for a location: erase + re-create
        lists.setdefault(c, []).append([s, e])
        prev = c
    return {c: v for c, v in lists.items() if 0 <= c[0] < m["dimx"] and 0 <= c[1] < m["dimy"]}


def reference_intervals(case):
    """The case's intervals as oracle.sipp_single_counted takes them: one run of consecutive entries per location."""
    if case["form"] == "job":
        return case["intervals"]
    return [[c[0], c[1], s, e] for c, v in cell_lists(case).items() for s, e in v]


def tier_of(traj, arena_nodes):
    """(tier, index of the first hand-over or None, index of the second or None) from the trajectory (module docstring)."""
    if len(traj) == 0:
        return 0, None, None
    nodes, opn = traj[:, 0].astype(np.int64), traj[:, 1].astype(np.int64)
    first_nodes = nodes + ROOM > LDS_NODES - 1
    first_open = opn + ROOM > LDS_NODES
    assert not (first_open & ~first_nodes).any()   # open <= nodes: the open condition never fires alone
    hit = np.nonzero(first_nodes | first_open)[0]
    if len(hit) == 0:
        return 0, None, None
    i0 = int(hit[0])
    hit2 = np.nonzero((opn[i0:] + ROOM > MIX_OPEN) | (nodes[i0:] + ROOM > arena_nodes))[0]
    if len(hit2) == 0:
        return 2, i0, None
    return 3, i0, i0 + int(hit2[0])


def classify(case):
    """Adds ref, K, S, travels, cls, expect, tier, why, near (module docstring)."""
    import oracle
    c, m, opt = case, case["map"], ENGINES[case["engine"]]
    cells = m["dimx"] * m["dimy"]
    assert cells <= opt["max_cells"] and c["form"] in FORMS, c["name"]
    safe = {cell: safe_from(v) for cell, v in cell_lists(c).items()}
    K, S = len(safe), sum(len(v) for v in safe.values())
    fits = all(len(v) <= SIPP_CAP and all(a < END_INF and (b == INT_MAX or b < END_INF) for a, b in v) for v in safe.values())
    travels = c["form"] != "resident" or not fits
    ref = oracle.sipp_single_counted(m["dimx"], m["dimy"], m["obstacles"], c["start"], c["goal"], reference_intervals(c),
                                     start_time=min(c["t0"], G_MAX), cap=PATH_CAP, traj_cap=TRAJ_CAP)
    assert ref["expanded"] <= TRAJ_CAP, c["name"]
    broken = []
    if c["t0"] > G_MAX:
        broken.append(("start time", "BAD_JOB"))
    if travels and (4 * ((cells + 1) // 2 + K + 1 + 2 * S) > TABLE_BYTES or
                    cells + S > opt["max_horizon"] * ((opt["max_cells"] + 31) // 32)):
        broken.append(("table", "CAP_NODES"))
    if ref["max_arrival"] > G_MAX:
        broken.append(("arrival", "CAP_HORIZON"))
    if ref["success"] and 2 * ref["raw_states"] > opt["max_horizon"]:
        broken.append(("path", "CAP_HORIZON"))
    if ref["created"] > opt["arena_nodes"]:
        broken.append(("nodes", "CAP_NODES"))
    why = "t0=%d K=%d S=%d travels=%s max_arrival=%d raw_states=%d created=%d max_open=%d@%d dk=%d" % (
        c["t0"], K, S, travels, ref["max_arrival"], ref["raw_states"], ref["created"], ref["max_open"],
        ref["nodes_at_max_open"], ref["decrease_keys"])
    c.update(ref=ref, K=K, S=S, travels=travels, expect=None, tier=None, near=None)
    if broken:
        assert len(broken) == 1, ("beyond two limits", c["name"], broken)
        c.update(cls="outside", expect=broken[0][1], why="%s: %s" % (broken[0][0], why))
        return c
    if not ref["success"]:
        assert ref["max_arrival"] < G_MAX, c["name"]  # no node of g = 1023 exists, so none is expanded (module docstring)
    if travels or (ref["expanded"] == 0 and not ref["success"]):
        tier, near = 1, None
    else:
        tier, i0, i1 = tier_of(ref["traj"], opt["arena_nodes"])
        nodes, opn = ref["traj"][:, 0], ref["traj"][:, 1]
        # how close the trajectory came to the hand-over that decided its tier: (condition, side, distance)
        near = []
        if tier == 0 and len(nodes) and LDS_NODES - 1 - ROOM - int(nodes.max()) < NEAR:
            near.append(("lds_nodes", "below"))
        if i0 is not None and int(nodes[i0]) - (LDS_NODES - 1 - ROOM) <= NEAR:
            near.append(("lds_nodes", "above"))
        if tier == 2 and MIX_OPEN - ROOM - int(opn[i0:].max()) < NEAR:
            near.append(("mix_open", "below"))
        if i1 is not None and int(opn[i1]) - (MIX_OPEN - ROOM) <= NEAR and int(nodes[i1]) + ROOM <= opt["arena_nodes"]:
            near.append(("mix_open", "above"))
    c.update(cls="inside", tier=tier, near=near, why=why)
    return c


# ---- the corpus -----------------------------------------------------------------------------------------------------------
def _case(group, name, engine, form, m, start, goal, intervals=(), t0=0, pre=None):
    return dict(name="%s/%s/%s" % (group, name, form), group=group, engine=engine, form=form, map=m, start=list(start),
                goal=list(goal), t0=int(t0), intervals=[[int(v) for v in iv] for iv in intervals], pre=pre)


def _forms(group, name, engine, m, start, goal, intervals=(), t0=0, forms=FORMS):
    return [_case(group, name, engine, f, m, start, goal, intervals, t0) for f in forms]


def _geometry_intervals(m, s, g, rng, near):
    """Collision intervals of one geometry case: on the unconstrained path (a wait), on the goal behind the earliest arrival
    (arrive later), on the far corner, the last row and the last column (one pair adjacent: no safe interval between), and
    on eight random cells near the start.  One list per cell, intervals of a cell disjoint."""
    import oracle
    dimx, dimy = m["dimx"], m["dimy"]
    plain = oracle.sipp_single_counted(dimx, dimy, m["obstacles"], s, g, [], cap=PATH_CAP)
    assert plain["success"]
    st = plain["states"]
    lists = {}
    if len(st) >= 3:
        t, x, y = st[len(st) // 2]
        lists[(x, y)] = [[t, t + 2]]
    if tuple(g) != tuple(s):
        lists.setdefault(tuple(g), []).append([plain["cost"] + 1, plain["cost"] + 2])
    border = (((dimx - 1, dimy - 1), [[0, 4], [9, 12], [13, 15]]), ((dimx // 2, dimy - 1), [[3, 5]]),
              ((dimx - 1, dimy // 2), [[2, 2], [6, 8]]))
    for cell, ivs in border:
        if cell not in lists and cell != tuple(s):
            lists[cell] = ivs
    d = lc.table(m, s)
    ring = [(x, y) for y in range(dimy) for x in range(dimx) if 0 < d[y, x] <= near]
    for _ in range(8):
        if not ring:
            break
        cell = ring[int(rng.integers(0, len(ring)))]
        if cell in lists:
            continue
        t, ivs = int(rng.integers(0, 30)), []
        for _ in range(int(rng.integers(1, 4))):
            a = t + int(rng.integers(0, 5))
            b = a + int(rng.integers(0, 4))
            ivs.append([a, b])
            t = b + 1 + int(rng.integers(0, 3))   # + 0: adjacent to the previous one
        lists[cell] = ivs
    return [[c[0], c[1], a, b] for c, v in lists.items() for a, b in v]


def _geometry_cases(rng):
    out = []
    for k, (dx, dy) in enumerate(GEOMETRY_DIMS):
        tag = "%dx%d" % (dx, dy)
        m = lc.geometry_map(dx, dy, 700 + k)
        engine = "big" if dx * dy > ENGINES["std"]["max_cells"] else "std"
        if dx * dy == 1:
            out += _forms("geometry", tag + "/stay", engine, m, [0, 0], [0, 0])
            out += _forms("geometry", tag + "/interval_ends", engine, m, [0, 0], [0, 0], [[0, 0, 2, 3]])  # [0, 1] is not a goal interval
            out += _forms("geometry", tag + "/blocked_at_t0", engine, m, [0, 0], [0, 0], [[0, 0, 0, 3]])
            continue
        near = 20
        origin = lc.table(m, [0, 0])
        free = [[x, y] for y in range(dy) for x in range(dx) if origin[y, x] < lc.INF]
        goals = [None, None, [int(rng.integers(0, dx)), dy - 1], [dx - 1, int(rng.integers(0, dy))], [dx - 1, dy - 1]]
        for j, g in enumerate(goals):
            if g is None:
                g = free[int(rng.integers(0, len(free)))]
            d = lc.table(m, g)
            ring = [c for c in free if 0 < d[c[1], c[0]] <= near]
            s = ring[int(rng.integers(0, len(ring)))]
            out += _forms("geometry", "%s/%d" % (tag, j), engine, m, s, g, _geometry_intervals(m, s, g, rng, near))
    return out


def _spread_intervals(rng, dimx, dimy, n_cells, t_max, avoid, t_min=0):
    """`n_cells` random cells with two to four short collision intervals each (at most five safe intervals), the first
    one starting in [t_min, t_max + 5]."""
    lists = {}
    while len(lists) < n_cells:
        cell = (int(rng.integers(0, dimx)), int(rng.integers(0, dimy)))
        if cell in lists or cell in avoid:
            continue
        t, ivs = int(rng.integers(t_min, t_max)), []
        for _ in range(int(rng.integers(2, 5))):
            a = t + int(rng.integers(0, 6))
            b = a + int(rng.integers(0, 3))
            ivs.append([a, b])
            t = b + 2 + int(rng.integers(0, 4))
        lists[cell] = ivs
    return [[c[0], c[1], a, b] for c, v in lists.items() for a, b in v]


TIER_QUOTA = 22


def _tier_cases(rng):
    """Resident cases on an open 64 x 64 map whose cells carry short collision intervals; the goal is blocked for a while in
    most of them, so the search spreads.  Candidates are classified as they come and kept until every tier has its quota.
    The open list of such a flood is its rim, a few hundred entries: the candidates meant for tier 3 also carry collision
    intervals BEHIND the search's time scale on 1500 cells, whose later safe intervals are generated with every cell the
    flood reaches and stay in the open list."""
    m = dict(dimx=64, dimy=64, obstacles=[])
    got = {0: [], 2: [], 3: []}
    late = None
    for k in range(600):
        if all(len(v) >= TIER_QUOTA for v in got.values()):
            break
        want = min(got, key=lambda t: len(got[t]))
        s = [int(rng.integers(8, 56)), int(rng.integers(8, 56))]
        reach = {0: 8, 2: 16, 3: 24}[want]
        g = [min(63, max(0, s[0] + int(rng.integers(-reach, reach + 1)))), min(63, max(0, s[1] + int(rng.integers(-reach, reach + 1))))]
        if g == s:
            continue
        ivs = _spread_intervals(rng, 64, 64, 300, 40, {tuple(s), tuple(g)})
        if want == 3:
            if late is None:
                late = _spread_intervals(rng, 64, 64, 1500, 100, set(), t_min=60)
            have = {(v[0], v[1]) for v in ivs} | {tuple(s), tuple(g)}
            ivs += [v for v in late if (v[0], v[1]) not in have]
        dist = abs(s[0] - g[0]) + abs(s[1] - g[1])
        hold = dist + int(rng.integers({0: 0, 2: 0, 3: 12}[want], {0: 6, 2: 12, 3: 22}[want]))
        ivs.append([g[0], g[1], 0, hold])
        c = classify(_case("tiers", "open64/%d" % k, "std", "resident", m, s, g, ivs))
        if c["cls"] == "inside" and c["tier"] in got and len(got[c["tier"]]) < TIER_QUOTA and c["ref"]["expanded"] <= 20000:
            got[c["tier"]].append(c)
    return [c for t in (0, 2, 3) for c in got[t]]


def comb(m_side, hold):
    """The comb of the module docstring on 255 x 3: corridor row 1 from the start (1, 1) to the right, the goal (0, 1) on the
    left blocked during [0, hold - 1]; every cell (x, 0), x >= 1, is a side cell blocked [0, 899] with m_side safe intervals
    from 900 on; row 2 and (0, 0) are obstacles.  Corridor cell x has f = 2 x - 1: it is expanded iff that is below `hold`."""
    dimx = 255
    m = dict(dimx=dimx, dimy=3, obstacles=[[x, 2] for x in range(dimx)] + [[0, 0]])
    ivs = [[0, 1, 0, hold - 1]]
    for x in range(1, dimx):
        ivs.append([x, 0, 0, 899])
        for q in range(1, m_side):
            ivs.append([x, 0, 899 + 3 * q, 900 + 3 * q])   # safe [900, 901], [904, 904] ... and the last one to INT_MAX
    return m, ivs


def comb_walk(m_side):
    """The same comb walked to its far end: start (1, 1), goal (254, 1), nothing blocked.  Every corridor cell has f = 253,
    so the search runs straight down the corridor and the path holds every node it expanded — the ones created just before
    a hand-over (the corridor cell is the last successor of its expansion) and just behind it included."""
    m, ivs = comb(m_side, 1)
    return m, ivs[1:]


def _handover_cases():
    """On both sides of the two hand-overs, within NEAR: for each side-list length the largest block time that stays below
    and the smallest that goes over (the trajectory is monotone in it)."""
    out = []
    for m_side, key in ((2, "lds_nodes"), (3, "lds_nodes"), (4, "lds_nodes"), (5, "mix_open"), (6, "mix_open"), (7, "mix_open")):
        below = above = None
        maps = {}
        for hold in range(21, 507, 2):
            m, ivs = comb(m_side, hold)
            m = maps.setdefault("m", m)   # one map object per family (the device test uploads it once)
            c = classify(_case("tiers", "comb%d/hold%d" % (m_side, hold), "std", "resident", m, [1, 1], [0, 1], ivs))
            if (key, "below") in (c["near"] or ()):
                below = c
            if (key, "above") in (c["near"] or ()):
                above = c
                break
        assert below is not None and above is not None, (m_side, key)
        out += [below, above]
    for m_side in (3, 6):   # one hand-over (tier 2) and both (tier 3), with the whole path across them
        m, ivs = comb_walk(m_side)
        out.append(classify(_case("tiers", "comb%d/walk" % m_side, "std", "resident", m, [1, 1], [254, 1], ivs)))
    return out


def list_of(n):
    """Collision intervals that leave exactly n safe intervals: [0, 1], [3, 3], [5, 5], ... and the last one to INT_MAX
    (n = 1: [1, INT_MAX])."""
    if n == 1:
        return [[0, 0]]
    return [[2 * k, 2 * k] for k in range(1, n)]


def gate_map():
    """5 x 3, the middle row a passage: S = (0, 1), L = (1, 1) is the only free cell of its column, M = (2, 1), G = (4, 1)."""
    return dict(dimx=5, dimy=3, obstacles=[[1, 0], [1, 2]])


S_, L_, M_, G_ = [0, 1], [1, 1], [2, 1], [4, 1]


def _table_cases():
    m = gate_map()
    out = []

    def on(cell, ivs):
        return [[cell[0], cell[1], a, b] for a, b in ivs]
    for n in RESIDENT_LISTS + LONG_LISTS:
        # M is blocked until the start of L's last finite interval: the path must use that interval of L
        safe = safe_from(list_of(n))
        j = len(safe) - 2 if n >= 3 else len(safe) - 1
        gate = on(M_, [[0, safe[j][0]]])
        ivs = gate + on(L_, list_of(n))
        forms = FORMS if n in RESIDENT_LISTS else ("job", "table")
        out += _forms("tables", "list%d" % n, "std", m, S_, G_, ivs, forms=forms)
        if n in RESIDENT_LISTS:   # L's list arrives as a delta record behind a warm-up job on the table
            out.append(_case("tables", "list%d_delta" % n, "std", "resident", m, S_, G_, ivs, pre=len(gate)))
    out += _forms("tables", "adjacent", "std", m, S_, G_, on(L_, [[2, 4], [5, 7]]) + on(M_, [[0, 5]]))
    out += _forms("tables", "from_zero", "std", m, S_, G_, on(L_, [[0, 3]]))
    out += _forms("tables", "start_blocked_forever", "std", m, S_, G_, on(S_, [[0, INT_MAX]]))
    out += _forms("tables", "goal_blocked_forever", "std", m, S_, G_, on(G_, [[0, INT_MAX]]))
    out += _forms("tables", "passage_blocked_forever", "std", m, S_, G_, on(L_, [[0, INT_MAX]]))
    out += _forms("tables", "t0_inside_collision", "std", m, S_, G_, on(S_, [[3, 6]]) + on(L_, [[1, 1]]), t0=4)
    out += _forms("tables", "unsorted", "std", m, S_, G_, on(L_, [[6, 6], [2, 2], [4, 4]]) + on(M_, [[0, 5]]))
    # the later list of L wins: [0, 3] alone (with both, L would be closed during [0, 3] AND [5, 9])
    out.append(_case("tables", "location_twice", "std", "job", m, S_, G_, on(L_, [[5, 9]]) + on(M_, [[0, 1]]) + on(L_, [[0, 3]])))
    return out


def _node_cases():
    """arena_nodes = 4096: the goal, next to the start on an open 64 x 64 map whose cells carry short collision intervals,
    is blocked so long that the search floods about 4000 nodes; three cells next to the start then get late safe intervals
    (from 601 on: generated by the first expansion, never expanded), one node each, until the reference creates exactly
    4096 nodes.  One more late interval, or one more step of waiting, is beyond the arena."""
    m = dict(dimx=64, dimy=64, obstacles=[])
    s, g, side = [32, 32], [33, 32], ([31, 32], [32, 33], [32, 31])
    spread = _spread_intervals(np.random.default_rng(911), 64, 64, 300, 40, {tuple(c) for c in (s, g) + side})
    an = ENGINES["small"]["arena_nodes"]

    def make(name, hold, extra, form="job"):
        ivs = spread + [[g[0], g[1], 0, hold - 1]]
        for k, cell in enumerate(side):
            n = max(0, min(extra - 120 * k, 120))
            ivs += [[cell[0], cell[1], 598 + 2 * q, 598 + 2 * q] for q in range(1, n + 1)]   # safe [0, 599], [601, 601], ...
        return classify(_case("limits", name, "small", form, m, s, g, ivs))
    hold, base = 10, None
    while True:   # the largest block time whose flood alone stays below the arena
        c = make("probe", hold + 1, 0)
        if c["ref"]["created"] >= an:
            break
        hold, base = hold + 1, c["ref"]["created"]
    assert base is not None and 0 < an - base <= 360, (hold, base)
    out = []
    for form in ("job", "table"):
        out.append(make("nodes_exact", hold, an - base, form))
        out.append(make("nodes_one_more_interval", hold, an - base + 1, form))
        out.append(make("nodes_one_more_step", hold + 1, an - base, form))
    return out


def _limit_cases():
    out = []
    line = dict(dimx=2, dimy=1, obstacles=[])
    for engine, forms in (("std", FORMS), ("long", ("job",))):
        out += _forms("limits", "arrival_1023_%s" % engine, engine, line, [0, 0], [1, 0], [[1, 0, 0, 1022]], forms=forms)
        out += _forms("limits", "arrival_1024_%s" % engine, engine, line, [0, 0], [1, 0], [[1, 0, 0, 1023]], forms=forms)
    row = dict(dimx=3, dimy=1, obstacles=[])
    out += _forms("limits", "late_interval_1023", "std", row, [1, 0], [2, 0], [[0, 0, 5, 1022]])
    out += _forms("limits", "late_interval_1024", "std", row, [1, 0], [2, 0], [[0, 0, 5, 1023]])
    out += _forms("limits", "t0_1023", "std", line, [0, 0], [0, 0], [[1, 0, 3, 4]], t0=1023)
    out += _forms("limits", "t0_1024", "std", line, [0, 0], [0, 0], [[1, 0, 3, 4]], t0=1024)
    snake = lc.serpentine(64, 33)
    for engine in ("std", "long"):
        half = ENGINES[engine]["max_horizon"] // 2
        for states in (half, half + 1):
            g = lc.corridor_cell(snake, [0, 0], states - 1)
            out += _forms("limits", "raw_path_%d_%s" % (states, engine), engine, snake, [0, 0], g)
    out += _node_cases()
    # travelling-table size, the byte condition: on 255 x 255 the cell index alone takes 32513 of the 32768 words
    big = lc.geometry_map(255, 255, 709)
    for name, k_cells in (("table_bytes_fit", 50), ("table_bytes_over", 51)):
        # 50 cells: 48 with two safe intervals + 2 with three: K + 2 S = 50 + 204 = 254; 51 cells with two: 51 + 204 = 255
        ivs = []
        for q in range(k_cells):
            cell = [200 + q % 10, 100 + q // 10]
            ivs.append([cell[0], cell[1], 4, 6])
            if k_cells == 50 and q < 2:
                ivs.append([cell[0], cell[1], 9, 9])
        s = [0, 250]
        out += _forms("limits", name, "big", big, s, [6, 254], ivs)
    # ... and the status-word condition: 8 x 8 with max_cells = 64 has 512 * 2 status words; 64 + S <= 1024
    small8 = dict(dimx=8, dimy=8, obstacles=[])
    for name, total in (("table_states_fit", 960), ("table_states_over", 961)):
        ivs, left = [], total
        for q in range(8, 64):   # rows 1 .. 7; the search runs along row 0
            n = min(left, 18)
            if n == 0:
                break
            if 0 < left - n < 2:
                n -= 1
            ivs += [[q % 8, q // 8, a, b] for a, b in ([[0, 0]] if n == 1 else [[2 * k, 2 * k] for k in range(1, n)])]
            left -= n
        assert left == 0
        out += _forms("limits", name, "tiny", small8, [0, 0], [7, 0], ivs, forms=("job", "table"))
    # resident bound: a far cell's safe interval starts at 65534 (resident) / 65535 (travels whole); the search never sees it
    open64 = dict(dimx=64, dimy=64, obstacles=[])
    for bound in (65534, 65535):
        out.append(_case("limits", "resident_bound_%d" % bound, "std", "resident", open64, [2, 2], [6, 3],
                         [[60, 60, 10, bound - 1], [4, 2, 1, 2]]))
    return out


_corpus = None


def corpus():
    """Every case, classified; built once per process."""
    global _corpus
    if _corpus is not None:
        return _corpus
    rng = np.random.default_rng(20241018)
    cases = [classify(c) for c in _geometry_cases(rng)]
    cases += _tier_cases(rng) + _handover_cases()
    cases += [classify(c) for c in _table_cases()]
    cases += [c if "cls" in c else classify(c) for c in _limit_cases()]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    _corpus = cases
    return _corpus
