"""The cases of the MRP_LL_JOB_TABLE_H tests (CPU: tests/test_table_h_cpu.py; device: tests/test_table_h_gpu.py): small
searches at the places where a table heuristic differs from the Manhattan one or meets a limit.  Every table is
heuristic_inputs.bfs — a plain BFS on the host —, every expected answer tests/support/table_h_check.cpp's, computed once.

  wall              8 x 8, a wall across the straight line with its gap at the far edge: Manhattan and table differ in `expanded`
  goal_constraints  wall + vertex constraints on the goal cell (m_lastGoalConstraint) + two edge constraints on the optimal path
  focal             A*-epsilon at w = 1.3, three context agents crossing the path
  focal_wide        the same with a context of 64 padded time steps x 32 padded agents (a 4096-byte focal table)
  h0_over           16 x 16 serpentine, h(start) = 134 > 124
  f_over            the same map, h(start) = 120, vertex constraints that force waits: f reaches 125 at t = 5
  horizon           the same map, h(start) = 70, no constraints
  big               48 x 48: table rows of dimx halfwords
  unreachable       goal walled in: MRP_LL_NO_SOLUTION, expanded == 0
  initial_cost      wall as MRP_LL_ASTAR with initial_cost = 7
"""
import functools

import heuristic_inputs
import table_h_checker as checker

INF = heuristic_inputs.INF
W = 1.3


def wall_map():
    return dict(dimx=8, dimy=8, obstacles=[[4, y] for y in range(7)])


def serpentine16():
    """Walls on the odd rows, gaps alternating between the last and the first column: (0, 0) to (0, 14) is 134 steps."""
    obst = [[x, y] for y in range(1, 14, 2) for x in range(16) if x != (15 if (y // 2) % 2 == 0 else 0)]
    return dict(dimx=16, dimy=16, obstacles=obst)


def table_of(m, goal):
    return heuristic_inputs.bfs(m["dimx"], m["dimy"], m["obstacles"], goal)


def cell_with_h(m, table, h):
    for y in range(m["dimy"]):
        for x in range(m["dimx"]):
            if int(table[y, x]) == h:
                return [x, y]
    raise AssertionError("no cell with h = %d" % h)


def _case(name, m, start, goal, vc=(), ec=(), ctx=(), agent=0, initial_cost=0, algos=(0, 1), tier=None):
    """tier: where the search ends under the default tier limits (4096 bytes of path area): 0 = in the narrow LDS tier, 1 = in
    the arena tier (a map beyond 32 x 32, an f beyond 124, more time steps than the tier has, or answered before any tier)."""
    return dict(name=name, map=m, start=list(start), goal=list(goal), vc=[list(v) for v in vc], ec=[list(e) for e in ec], w=W,
                agent=agent, ctx=[[list(xy) for xy in p] for p in ctx], cap=-1, initial_cost=initial_cost, algos=tuple(algos),
                tier=tier, table=table_of(m, goal))


def expected(algo, c):
    """The checker's answer for case c run as algo (0 = MRP_LL_ASTAR, 1 = MRP_LL_ASTAR_EPS)."""
    return checker.ll_search(algo, c["map"], c["start"], c["goal"], c["table"], c["vc"], c["ec"], w=c["w"], agent_idx=c["agent"],
                             ctx_paths=c["ctx"] if algo == 1 else (), cap_expansions=c["cap"],
                             initial_cost=c["initial_cost"] if algo == 0 else 0)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    wm = wall_map()
    wall = _case("wall", wm, [1, 1], [6, 1], tier=0)
    out.append(wall)
    path = [s[1:] for s in expected(0, wall)["states"]]  # the optimal path's cells
    assert len(path) == 18
    T = len(path) - 1
    out.append(_case("goal_constraints", wm, [1, 1], [6, 1], vc=[[T, 6, 1], [T + 2, 6, 1]],
                     ec=[[3] + path[3] + path[4], [9] + path[9] + path[10]], tier=0))
    crossing = [[], [path[2]] * 6, [path[k] for k in range(7, 0, -1)], [path[5]] * 10]
    out.append(_case("focal", wm, [1, 1], [6, 1], ctx=crossing, tier=0))
    wide = [p + [p[-1]] * (64 - len(p)) if p else [] for p in crossing] + [[[7, k % 8]] * 64 for k in range(16)]
    assert len(wide) == 20 and max(len(p) for p in wide) == 64
    out.append(_case("focal_wide", wm, [1, 1], [6, 1], ctx=wide, tier=0))
    sm = serpentine16()
    goal = [0, 14]
    tab = table_of(sm, goal)
    assert int(tab[0, 0]) == 134
    out.append(_case("h0_over", sm, [0, 0], goal, tier=1))
    s120 = cell_with_h(sm, tab, 120)
    nxt = [c for c in ([s120[0] + 1, s120[1]], [s120[0] - 1, s120[1]], [s120[0], s120[1] + 1], [s120[0], s120[1] - 1])
           if 0 <= c[0] < 16 and 0 <= c[1] < 16 and int(tab[c[1], c[0]]) == 119]
    assert len(nxt) == 1
    out.append(_case("f_over", sm, s120, goal, vc=[[t] + nxt[0] for t in range(1, 7)], tier=1))
    out.append(_case("horizon", sm, cell_with_h(sm, tab, 70), goal, tier=1))
    bm = heuristic_inputs.random_map(48, 48, 5)
    free = heuristic_inputs.free_cells(bm)
    bgoal = free[len(free) // 3]
    btab = table_of(bm, bgoal)
    far = max((c for c in free if int(btab[c[1], c[0]]) != INF), key=lambda c: (int(btab[c[1], c[0]]), c[1], c[0]))
    assert int(btab[far[1], far[0]]) >= 48
    out.append(_case("big", bm, far, bgoal, tier=1))
    um = dict(dimx=8, dimy=8, obstacles=[[5, 6], [7, 6], [6, 5], [6, 7]])
    unreach = _case("unreachable", um, [1, 1], [6, 6], tier=1)
    assert int(unreach["table"][1, 1]) == INF
    out.append(unreach)
    out.append(_case("initial_cost", wm, [1, 1], [6, 1], initial_cost=7, algos=(0,), tier=0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def runs():
    """[(algo, case, expected)] for every case in every algorithm it is run as."""
    return tuple((algo, c, expected(algo, c)) for c in cases() for algo in c["algos"])


# The driver test's sixteen 8 x 8, 12-obstacle instances (mrp_hl_generate_instances' generator): (seed, agents).  Chosen so
# that the Manhattan CBS and ECBS (w = 1.3) of the CPU oracle solve each within DRIVER_CAP low-level expansions — checked in
# tests/test_table_h_cpu.py; seed 8802 does not and is left out.
DRIVER_CAP = 20000
DRIVER_SEEDS = tuple((seed, 4 + k % 3) for k, seed in enumerate([8800, 8801] + list(range(8803, 8817))))


def driver_instances():
    from libmultirobotplanning_amd import hl
    return [hl.generate_instance(seed, 8, 8, 12, n_agents) for seed, n_agents in DRIVER_SEEDS]
