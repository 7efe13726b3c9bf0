"""Corpus and classifier of the limit tests (tests/test_limit_cases_cpu.py on the CPU, tests/test_ll_limits_gpu.py on the
device): low-level searches on large and non-square maps, and searches at the engine's documented capacity limits
(include/mrp_ll.h: MRP_LL_CAP_NODES, MRP_LL_CAP_HORIZON, MRP_LL_CAP_FOCAL).  CPU only: the engine is never imported.

A case is a dict: name, engine (a key of ENGINES), map, algo ("astar", "eps", "ta", "eps_ta"), start, goal (None: an agent
without a task), vc, ec, ctx, agent, w, heur ("upload": the test uploads a BFS table; "device": it lets the engine compute
it), group.  classify() adds ref (the reference's answer), T and N (the time-step and node limits the header documents
for that algorithm, map and option set), cls ("inside" / "outside" / "between"), expect (the capacity status of an outside
case, as the name of the constant) and why.

The references:
  astar, eps   oracle.ll_search            (a_star.hpp / a_star_epsilon.hpp over example/ecbs.cpp's Environment)
  ta           oracle.ta_ll_search         (a_star.hpp over example/cbs_ta.cpp's Environment)
  eps_ta       ecbs_ta_checker.ll_search   (a_star_epsilon.hpp over example/ecbs_ta.cpp's Environment); its `nodes` and
               `max_time` count GENERATED states (tests/support/ecbs_ta_check.cpp LLEnv::onDiscover: every state handed to
               the open list, the start included in `nodes`; max_time = the largest time of any of them).

The limits, as include/mrp_ll.h states them (an = arena_nodes, cells = dimx * dimy):
  astar, eps   T = max_horizon                              N = an
  ta           T = min(max_horizon, 4 * an / cells)         N = an            g <= 1023, f <= 2045
  eps_ta       B = 40 * an + 48
               T = min(max_horizon, B / (8 * cells))        N = (B - 4 * T * cells - 64) / 48
               g <= 1023, f <= 2045, focalH <= 2047
T counts time steps: states of time 0 .. T - 1 exist; a state of time T "would have been generated" -> MRP_LL_CAP_HORIZON.

The bounds the classes rest on.  Every one follows from the reference's semantics alone.

  (E) the largest time of a node the reference EXPANDS without ending the search there.  With F = floor(w * fmin) in
      binary32 (w = 1 for astar and ta): A* expands a node only with f <= fmin, A*-epsilon only out of the focal list, f <= w *
      bestFScore <= w * fmin (bestFScore follows the open list's top, which never falls with these consistent heuristics:
      Manhattan distance, the shortest-path table, 0).  A node on another cell than the goal has h >= 1, so g <= F - 1; a
      node on the goal cell that does not end the search has time <= lastGoal (m_lastGoalConstraint).
        astar, eps      time == g:  E = F - 1   (lastGoal < cost <= F, so the goal-cell nodes are covered)
        ta, eps_ta      a Wait on the goal cell is free, so time can run ahead of g.  Such a Wait is taken out of an expanded
                        goal-cell node, i.e. at a time tw <= lastGoal, and whoever stands on the goal cell has g >= d0 = the
                        table's value at the start.  A node n off the goal cell whose path holds such a Wait, the last one at tw:
                        time(n) = tw + 1 + g(n) - g(after the Wait) <= lastGoal + 1 + (F - 1) - d0.
                        E = max(F - 1, lastGoal + F - d0) with a goal constraint (lastGoal >= 0), else F - 1
        without a task  every state of time > lastGoal (the largest vertex-constraint time) ends the search:  E = lastGoal
        eps_ta also     E <= max_time (an expanded node was generated first)
        no path found   the open list runs empty only if the constraints kill every branch; one time step behind the last
                        constraint a Wait is always possible:  generated times <= largest constraint time + 2, E = that - 1
      Successors have time E + 1 at most, so the horizon HOLDS if E + 1 <= T - 1.
      It CANNOT hold if the reference's path contains a state of time >= T (astar, eps: cost >= T), or (eps_ta) max_time >=
      T, or (ta, eps_ta) the start's table value is beyond the f field (h0 > 2045, or no way to the task at all).
      (ta, eps_ta: "holds" also needs F + 2 <= 2045: a successor's f exceeds its expanded parent's, <= F, by at most 2 — one for
      g, one for h — and h <= f; without a path: E + 1 + hmax <= 2045, hmax = the table's largest finite value.  g <= time.)
  (N) nodes.  An expansion creates at most five nodes, so created <= 5 * expanded + 1 (eps_ta: the checker's `nodes`); the
      engine wants room for five more before an expansion:  HOLDS if created + 5 <= N.  Every expanded node was created, so
      it CANNOT hold if expanded > N (eps_ta: nodes > N).
  (Fh) focalH (eps, eps_ta).  focalH of a node = the sum over the steps of its path of focalStateHeuristic +
      focalTransitionHeuristic (ecbs.cpp:282-312, ecbs_ta.cpp:314-344; a_star_epsilon.hpp:231-235).  A step adds at most 2 per
      context agent, so focalH <= 2 * agents * (E + 1) — where that is too coarse, a dynamic programme over (time, cell)
      takes the maximum over ALL walks through states that bound (E) allows to be expanded (_focal_upper_bound).  HOLDS if
      that maximum is <= 2047.  It CANNOT hold if a node of the reference's own path has focalH > 2047 (_path_focal).

  inside    horizon, nodes and focalH all hold                      -> the engine equals the reference bit for bit
  outside   exactly one of the three cannot hold, the others hold   -> the engine returns that limit's status
  between   anything else                                           -> the exact answer, or CAP_NODES / CAP_HORIZON

The focalH cases: a 1 x (L + 1) corridor, agent 0 walks from x = 0 to x = L at w = 1.0 and sees n context agents whose
paths are that same walk.  Stepping right from (x, t) to (x + 1, t + 1) meets all n agents on the new cell at t + 1:
focalStateHeuristic (ecbs.cpp:282-295) = n; none of them moves against the step, focalTransitionHeuristic (ecbs.cpp:298-312)
= 0.  The start node has focalH 0 (a_star_epsilon.hpp:113), so the node (k, t = k) has focalH n * k and the goal node n * L.
Off that walk a node has f > L = fmin and is not expanded at w = 1.0."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import heuristic_inputs  # noqa: E402

INF = heuristic_inputs.INF
G_MAX, F_MAX, FH_MAX = 1023, 2045, 2047   # include/mrp_ll.h: g <= 1023, f <= 2045, focalH <= 2047
REF_CAP = 3_000_000                       # expansion cap of the references: no case comes near it (asserted)
PATH_CAP = 4200                           # room for the longest reference path (the 4000-step serpentine walk)

# the option sets (mrp_ll_options) of the engines the device test creates, defaults resolved as mrp_ll_create does
ENGINES = {
    # large maps: default arena and horizon; 16 slots keep the arena of 255 x 255 cells small
    "big": dict(slots=16, n_tickets=1, arena_nodes=131072, max_horizon=512, max_cells=65025, lds_nodes=0),
    # the g / horizon / f / h limits: the longest horizon and the largest arena the engine takes
    "long": dict(slots=2, n_tickets=1, arena_nodes=1 << 22, max_horizon=1024, max_cells=65025, lds_nodes=0),
    # no LDS tier and a small arena: the arena tier on small non-square maps, CAP_NODES, CAP_FOCAL
    "arena_only": dict(slots=64, n_tickets=1, arena_nodes=4096, max_horizon=512, max_cells=4096, lds_nodes=-1),
    # everything default: the compact tier must hand the focalH cases over, not wrap
    "default": dict(slots=64, n_tickets=1, arena_nodes=131072, max_horizon=512, max_cells=4096, lds_nodes=0),
}
ALGOS = ("astar", "eps", "ta", "eps_ta")


def limits(algo, opt, m):
    """(T, N) of include/mrp_ll.h for this algorithm, option set and map (module docstring)."""
    an, hz, cells = opt["arena_nodes"], opt["max_horizon"], m["dimx"] * m["dimy"]
    if algo in ("astar", "eps"):
        return hz, an
    if algo == "ta":
        return min(hz, 4 * an // cells), an
    b = 40 * an + 48
    t = min(hz, b // (8 * cells))
    return t, (b - 4 * t * cells - 64) // 48


def _f32_floor(w, f):
    return int(np.float32(f) * np.float32(w))  # int * float in binary32, as a_star_epsilon.hpp:240 computes the bound


def _pos(path, t):
    return path[t] if t < len(path) else path[-1]


def _path_focal(case, states):
    """The largest focalH along the reference's own path: per step focalStateHeuristic (agents on the new cell at the new
    time) + focalTransitionHeuristic (agents that were on the new cell and now are on the old one), ecbs.cpp:282-312."""
    others = [p for i, p in enumerate(case["ctx"]) if i != case["agent"] and len(p)]
    fh = best = 0
    for a, b in zip(states, states[1:]):
        for p in others:
            pa, pb = _pos(p, a[0]), _pos(p, b[0])
            fh += (pb[0] == b[1] and pb[1] == b[2]) + (pa[0] == b[1] and pa[1] == b[2] and pb[0] == a[1] and pb[1] == a[2])
        best = max(best, fh)
    return best


_MOVES = ((0, 0), (-1, 0), (1, 0), (0, 1), (0, -1))


def _shift(a, dx, dy, fill):
    """out[y + dy, x + dx] = a[y, x]"""
    out = np.full_like(a, fill)
    h, w = a.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = a[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def _focal_upper_bound(case, e_max, f_max, slack, h, last_goal):
    """The largest focalH of any node that can be generated: maximum over all walks from the start whose expanded states
    satisfy bound (E) — free cell, time <= e_max, time - slack + h(cell) <= f_max, not a goal-cell state of time >
    last_goal.  Constraints are ignored (a superset of the reference's walks)."""
    m = case["map"]
    dimx, dimy = m["dimx"], m["dimy"]
    free = np.ones((dimy, dimx), dtype=bool)
    for o in m["obstacles"]:
        free[o[1], o[0]] = False
    others = [p for i, p in enumerate(case["ctx"]) if i != case["agent"] and len(p)]
    val = np.full((dimy, dimx), -1, dtype=np.int64)
    val[case["start"][1], case["start"][0]] = 0
    best = 0
    for t in range(e_max + 1):
        exp = (val >= 0) & (t - slack + h <= f_max)
        if case["goal"] is not None and t > last_goal:
            exp[case["goal"][1], case["goal"][0]] = False
        if not exp.any():
            break
        vert = np.zeros((dimy, dimx), dtype=np.int64)
        for p in others:
            b = _pos(p, t + 1)
            vert[b[1], b[0]] += 1
        new = np.full((dimy, dimx), -1, dtype=np.int64)
        for dx, dy in _MOVES:
            edge = np.zeros((dimy, dimx), dtype=np.int64)  # indexed by the cell the step leaves
            for p in others:
                a, b = _pos(p, t), _pos(p, t + 1)
                sx, sy = b[0], b[1]
                if a[0] == sx + dx and a[1] == sy + dy:
                    edge[sy, sx] += 1
            cand = _shift(np.where(exp, val + edge, -1), dx, dy, -1)
            cand = np.where((cand >= 0) & free, cand + vert, -1)
            new = np.maximum(new, cand)
        val = new
        best = max(best, int(val.max()))
    return best


def reference(case):
    import oracle
    m, c = case["map"], case
    if c["algo"] == "astar":
        r = oracle.ll_search(oracle.ASTAR, m, c["agent"], c["start"], c["goal"], c["vc"], c["ec"], [], w=1.0,
                             cap_expansions=REF_CAP, cap=PATH_CAP)
    elif c["algo"] == "eps":
        r = oracle.ll_search(oracle.ASTAR_EPS, m, c["agent"], c["start"], c["goal"], c["vc"], c["ec"], c["ctx"], w=c["w"],
                             cap_expansions=REF_CAP, cap=PATH_CAP)
    elif c["algo"] == "ta":
        r = oracle.ta_ll_search(m, c["start"], c["goal"], c["vc"], c["ec"], cap_expansions=REF_CAP, cap=PATH_CAP)
    else:
        import ecbs_ta_checker
        r = ecbs_ta_checker.ll_search(m, c["start"], c["goal"], c["vc"], c["ec"], w=c["w"], agent_idx=c["agent"],
                                      ctx_paths=c["ctx"], cap_expansions=REF_CAP, cap=PATH_CAP)
    assert r["rc"] != -1, ("the reference ran into its expansion cap", c["name"])
    return r


_tables = {}


def table(m, goal):
    """The goal's shortest-path table (shortest_path_heuristic.hpp), int64 [dimy][dimx], INF = unreachable; cached."""
    key = (id(m), tuple(goal))
    if key not in _tables:
        _tables[key] = heuristic_inputs.bfs(m["dimx"], m["dimy"], m["obstacles"], goal)
    return _tables[key]


def classify(case):
    """Adds ref, T, N, cls, expect, why (module docstring)."""
    c, m = case, case["map"]
    algo = c["algo"]
    ta = algo in ("ta", "eps_ta")
    focal = algo in ("eps", "eps_ta")
    T, N = limits(algo, ENGINES[c["engine"]], m)
    ref = reference(c)
    w = c["w"] if focal else 1.0
    goal = c["goal"]
    vtimes = [v[0] for v in c["vc"]]
    if goal is None:
        last_goal = max(vtimes, default=-1)
    else:
        last_goal = max((v[0] for v in c["vc"] if v[1] == goal[0] and v[2] == goal[1]), default=-1)
    # ---- (E): horizon
    if goal is None:
        h = np.zeros((m["dimy"], m["dimx"]), dtype=np.int64)
    elif ta:
        h = table(m, goal)
    else:
        ys, xs = np.mgrid[0:m["dimy"], 0:m["dimx"]]
        h = np.abs(xs - goal[0]) + np.abs(ys - goal[1])
    slack = last_goal + 1 if ta else 0
    if ref["success"]:
        f_max = _f32_floor(w, ref["fmin"])
        if goal is None:
            e_max = last_goal
        elif ta and last_goal >= 0:
            e_max = max(f_max - 1, last_goal + f_max - int(h[c["start"][1], c["start"][0]]))
        else:
            e_max = f_max - 1
    else:
        f_max = 1 << 30
        e_max = max(vtimes + [e[0] for e in c["ec"]], default=-1) + 1
    if algo == "eps_ta":
        e_max = min(e_max, ref["max_time"])
    e_max = max(e_max, -1)
    hz_holds = e_max + 1 <= T - 1
    hz_fails = ref["success"] and ref["states"][-1][0] >= T
    if algo == "eps_ta" and ref["max_time"] >= T:
        hz_fails = True
    if ta:
        finite = h[h < INF]
        h0 = int(h[c["start"][1], c["start"][0]])
        if h0 > F_MAX:
            hz_fails = True
        if (f_max + 2 if ref["success"] else e_max + 1 + int(finite.max())) > F_MAX or e_max + 1 > G_MAX:
            hz_holds = False
    # ---- (N): nodes
    created = ref["nodes"] if algo == "eps_ta" else 5 * ref["expanded"] + 1
    nd_holds = created + 5 <= N
    nd_fails = (ref["nodes"] if algo == "eps_ta" else ref["expanded"]) > N
    # ---- (Fh): focalH
    fh_holds, fh_fails = True, False
    n_others = sum(1 for i, p in enumerate(c["ctx"]) if i != c["agent"] and len(p)) if focal else 0
    if n_others:
        fh_fails = ref["success"] and _path_focal(c, ref["states"]) > FH_MAX
        fh_holds = 2 * n_others * (e_max + 1) <= FH_MAX
        if not fh_holds and not fh_fails and m["dimx"] * m["dimy"] * (e_max + 1) <= 2_000_000:
            fh_holds = _focal_upper_bound(c, e_max, f_max, slack, h, last_goal) <= FH_MAX
    holds = dict(horizon=hz_holds, nodes=nd_holds, focal=fh_holds)
    fails = dict(horizon=hz_fails, nodes=nd_fails, focal=fh_fails)
    assert not any(holds[k] and fails[k] for k in holds), (c["name"], holds, fails)
    broken = [k for k in fails if fails[k]]
    c.update(ref=ref, T=T, N=N, expect=None)
    if all(holds.values()):
        c.update(cls="inside", why="E=%d T=%d created<=%d N=%d" % (e_max, T, created, N))
    elif len(broken) == 1 and all(holds[k] for k in holds if k != broken[0]):
        c.update(cls="outside", expect=dict(horizon="CAP_HORIZON", nodes="CAP_NODES", focal="CAP_FOCAL")[broken[0]],
                 why="%s cannot hold: E=%d T=%d created<=%d N=%d" % (broken[0], e_max, T, created, N))
    else:
        c.update(cls="between", why="holds=%r fails=%r E=%d T=%d created<=%d N=%d" % (holds, fails, e_max, T, created, N))
    return c


# ---- the corpus -----------------------------------------------------------------------------------------------------------
def _case(name, engine, m, algo, start, goal, vc=(), ec=(), ctx=(), w=1.0, heur="upload", group="geometry"):
    focal = algo in ("eps", "eps_ta")
    return dict(name="%s/%s/%s" % (group, name, algo), engine=engine, map=m, algo=algo, start=list(start),
                goal=None if goal is None else list(goal), vc=[list(v) for v in vc], ec=[list(e) for e in ec],
                ctx=[list(p) for p in ctx] if focal else [], agent=0, w=float(w) if focal else 1.0, heur=heur, group=group)


def geometry_map(dimx, dimy, seed):
    """About 20 % random obstacles (none where a dimension is 1); the first column, the last column and the last row are
    kept free, so the four corners lie in one component and the constraints on the last row / column sit on free cells."""
    if dimx == 1 or dimy == 1:
        return dict(dimx=dimx, dimy=dimy, obstacles=[])
    m = heuristic_inputs.random_map(dimx, dimy, seed)
    m["obstacles"] = [o for o in m["obstacles"] if o[0] not in (0, dimx - 1) and o[1] != dimy - 1]
    return m


def _border_walk(m, limit):
    """A context path along the last row, left to right, then up the last column (at most `limit` states)."""
    dimx, dimy = m["dimx"], m["dimy"]
    p = [[x, dimy - 1] for x in range(dimx)] + [[dimx - 1, y] for y in range(dimy - 2, -1, -1)]
    return p[:limit]


def _geometry_cases(engine, m, tag, rng, n_random, near, far_pairs=True):
    """Searches of all four algorithms on one map: corner to corner (where the distance leaves the search short), random free
    cells `near` steps apart, each once plain and once under constraints: a vertex and an edge constraint on the unconstrained
    path (a detour), a constraint on the goal cell (the agent arrives and must outlast it), constraints on the last row, the
    last column and the far-corner cell at times up to max_horizon - 1, and edge constraints whose move leaves the grid on all
    four sides.  The focal algorithms see two context agents walking the last row and column in opposite directions."""
    import oracle
    opt = ENGINES[engine]
    dimx, dimy, hz = m["dimx"], m["dimy"], opt["max_horizon"]
    far = [dimx - 1, dimy - 1]
    corners = [[0, 0], [dimx - 1, 0], [0, dimy - 1], far]
    from_origin = table(m, [0, 0])
    free = [[x, y] for y in range(dimy) for x in range(dimx) if from_origin[y, x] < INF]
    pairs = []
    if far_pairs:
        pairs += [(corners[0], far), (far, corners[0]), (corners[1], far), (corners[2], far)]
    else:  # a map whose corners are too far apart for a short search: from each corner to a cell nearby
        for cn in corners:
            d = table(m, cn)
            ring = [c for c in free if 0 < d[c[1], c[0]] <= near]
            pairs.append((cn, ring[int(rng.integers(0, len(ring)))]))
            pairs.append((ring[int(rng.integers(0, len(ring)))], cn))
    for _ in range(n_random):
        s = free[int(rng.integers(0, len(free)))]
        d = table(m, s)
        ring = [c for c in free if d[c[1], c[0]] <= near]
        pairs.append((s, ring[int(rng.integers(0, len(ring)))]))
    walk = _border_walk(m, hz - 2)
    ctx = [[], walk, walk[::-1]]
    late = [[hz - 1, far[0], far[1]], [hz - 1, 0, dimy - 1], [hz - 2, dimx - 1, 0], [hz // 2, dimx // 2, dimy - 1],
            [hz // 3, dimx - 1, dimy // 2]]
    out = []
    for k, (s, g) in enumerate(pairs):
        plain = oracle.ll_search(oracle.ASTAR, m, 0, s, g, cap_expansions=REF_CAP, cap=PATH_CAP)
        assert plain["success"]
        st = plain["states"]
        vc, ec = [], []
        if len(st) >= 3:
            a, b = st[len(st) // 2], st[len(st) // 2 + 1] if len(st) // 2 + 1 < len(st) else st[-1]
            vc.append([a[0], a[1], a[2]])
            ec.append([st[0][0], st[0][1], st[0][2], st[1][1], st[1][2]])
            ec.append([b[0] - 1, a[1], a[2], b[1], b[2]])
        vc.append([plain["cost"] + 1, g[0], g[1]])  # m_lastGoalConstraint: arrive, leave or wait, come back
        vc += [v for v in late if v[1:] != list(g)]  # (a late constraint on the goal cell would keep the reference busy forever)
        # edge constraints whose move leaves the grid (they can never match a move the search makes)
        ec += [[0, 0, s[1], -1, s[1]], [1, dimx - 1, s[1], dimx, s[1]], [0, s[0], 0, s[0], -1], [1, s[0], dimy - 1, s[0], dimy],
               [hz - 1, far[0], far[1], dimx, far[1]], [hz - 1, far[0], far[1], far[0], dimy]]
        for algo in ALGOS:
            w = 1.3 if k % 2 == 0 else 1.0
            out.append(_case("%s/%d_plain" % (tag, k), engine, m, algo, s, g, ctx=ctx, w=w))
            out.append(_case("%s/%d_constrained" % (tag, k), engine, m, algo, s, g, vc, ec, ctx=ctx, w=w))
    # an agent without a task: it must outlast its last vertex constraint
    s = free[int(rng.integers(0, len(free)))]
    for algo in ("ta", "eps_ta"):
        out.append(_case("%s/no_task" % tag, engine, m, algo, s, None, [[3, s[0], s[1]], [5, far[0], far[1]]], [], ctx=ctx, w=1.3))
    return out


def serpentine(dimx, dimy):
    """Obstacle rows at odd y with one gap, alternating between x = dimx - 1 and x = 0: one corridor from (0, 0)."""
    obst = [[x, y] for y in range(1, dimy, 2) for x in range(dimx) if x != (dimx - 1 if (y // 2) % 2 == 0 else 0)]
    return dict(dimx=dimx, dimy=dimy, obstacles=obst)


def corridor_cell(m, start, dist):
    """The cell at corridor distance `dist` from `start` (unique in a serpentine when start is the corridor's end)."""
    d = table(m, start)
    ys, xs = np.nonzero(d == dist)
    assert len(xs) == 1, (dist, len(xs))
    return [int(xs[0]), int(ys[0])]


def _horizon_cases():
    """g and horizon (engine "long": max_horizon 1024): the goal 1022, 1023 and 1024 corridor steps from (0, 0) on a 64 x 33
    serpentine; A*-epsilon at w = 1.3 and distance 786 (floor(1.3 * 786) + 1 = 1022 < 1024)."""
    m = serpentine(64, 33)
    out = []
    for d in (1022, 1023, 1024):
        g = corridor_cell(m, [0, 0], d)
        for algo in ("astar", "ta", "eps_ta") if d != 1024 else ALGOS:
            out.append(_case("d%d" % d, "long", m, algo, [0, 0], g, w=1.0, group="horizon"))
    out.append(_case("d786_w1.3", "long", m, "eps", [0, 0], corridor_cell(m, [0, 0], 786), w=1.3, group="horizon"))
    return out


def _field_cases():
    """f and h of the task-assignment searches (engine "long"): a 64 x 67 serpentine (a corridor of 2209 cells), the goal's
    table computed on the device, starts 2044, 2046 and 2048 + 30 corridor steps from the goal; and 4000 steps on a 64 x 125
    serpentine (the corridor of 64 x 67 is too short for it).  h0 = 2044 fits the f field and the search then runs out of time
    steps; the others do not fit (f <= 2045).  An h that wrapped in an 11-bit field would read 2046, 30 and 1952."""
    g = [0, 0]
    out = []
    for m, dists in ((serpentine(64, 67), (2044, 2046, 2048 + 30)), (serpentine(64, 125), (4000,))):
        for d in dists:
            s = corridor_cell(m, g, d)
            for algo in ("ta", "eps_ta"):
                out.append(_case("h%d" % d, "long", m, algo, s, g, w=1.0, heur="device", group="fields"))
    return out


FOCAL_NL = ((89, 23, True), (100, 20, True), (90, 23, False), (100, 21, False), (150, 14, False))  # (n, L, n * L <= 2047)


def _focal_cases():
    """focalH (module docstring): (n, L) context agents and corridor length; through the default engine (A*-epsilon: the
    compact tier hands over) and through the arena-only engine (A*-epsilon and the task-assignment form)."""
    out = []
    for n, L, _ in FOCAL_NL:
        m = dict(dimx=L + 1, dimy=1, obstacles=[])
        walk = [[x, 0] for x in range(L + 1)]
        ctx = [[]] + [walk] * n
        for engine, algos in (("default", ("eps",)), ("arena_only", ("eps", "eps_ta"))):
            for algo in algos:
                out.append(_case("n%d_L%d_%s" % (n, L, engine), engine, m, algo, [0, 0], [L, 0], ctx=ctx, w=1.0, group="focal"))
    return out


def _node_cases():
    """CAP_NODES (engine "arena_only": 4096 nodes): a vertex constraint on the goal cell six steps behind the earliest arrival
    on a 48 x 48 map: the reference expands 6 000 to 11 000 nodes of the waiting states around the path."""
    m = geometry_map(48, 48, 11)
    out = []
    for k, (s, g) in enumerate((([47, 0], [0, 47]), ([5, 3], [44, 30]))):
        d0 = int(table(m, g)[s[1], s[0]])
        for algo, w in (("astar", 1.0), ("eps", 1.3)):
            out.append(_case("wait%d" % k, "arena_only", m, algo, s, g, [[d0 + 6, g[0], g[1]]], w=w, group="nodes"))
    return out


_corpus = None


def corpus():
    """Every case, classified; built once per process."""
    global _corpus
    if _corpus is not None:
        return _corpus
    cases = []
    rng = np.random.default_rng(20240607)
    for k, (dx, dy) in enumerate(((33, 31), (31, 33), (48, 48), (100, 37), (37, 100), (64, 64), (255, 1), (1, 255), (255, 3))):
        # (end to end a 255-cell corridor is a long search at w = 1.3: from its corners to cells nearby instead)
        cases += _geometry_cases("big", geometry_map(dx, dy, 300 + k), "%dx%d" % (dx, dy), rng, n_random=2, near=30,
                                 far_pairs=min(dx, dy) > 3)
    # 255 x 255: corner to corner is 508 steps (inside the 512 of A* / A*-epsilon); the task-assignment searches get 8 and 10
    # time steps there, so the pairs are 3 to 12 steps apart: some inside, some outside
    big = geometry_map(255, 255, 399)
    cases += _geometry_cases("big", big, "255x255", rng, n_random=4, near=6, far_pairs=False)
    for s, g in (([254, 254], [254, 243]), ([243, 254], [254, 254]), ([0, 0], [0, 9]), ([254, 0], [245, 0])):
        for algo in ALGOS:
            cases.append(_case("255x255/far_%d_%d" % (s[0], s[1]), "big", big, algo, s, g, w=1.0))
    for k, (dx, dy) in enumerate(((31, 17), (17, 31), (32, 5), (1, 32), (1, 1))):
        m = geometry_map(dx, dy, 500 + k)
        if dx * dy == 1:
            for algo in ALGOS:
                cases.append(_case("1x1/stay", "arena_only", m, algo, [0, 0], [0, 0], w=1.3))
                cases.append(_case("1x1/outlast", "arena_only", m, algo, [0, 0], [0, 0], [[0, 0, 0]], w=1.3))
                # the constraint kills the only branch: the open list runs empty
                cases.append(_case("1x1/no_path", "arena_only", m, algo, [0, 0], [0, 0], [[1, 0, 0], [2, 0, 0]], w=1.3))
            continue
        cases += _geometry_cases("arena_only", m, "%dx%d" % (dx, dy), rng, n_random=1, near=12)
    cases += _horizon_cases() + _field_cases() + _focal_cases() + _node_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    _corpus = [classify(c) for c in cases]
    return _corpus
