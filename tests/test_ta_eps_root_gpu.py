"""mrp_ll_ta_eps_root_batch on the MI355X: the root node of an ECBS-TA conflict tree (ecbs_ta.hpp:117-138, :306-343) by one
workgroup, with ONE table in the arena slot as the next search's focal context and as the scan's input.

The yardstick is what the engine offers for the same work without the call, with the checker behind it
(tests/test_ecbs_ta_parity_gpu.py, tests/test_conflict_scan_gpu.py): the same agents as ordinary MRP_LL_ASTAR_EPS_TA jobs run
one after another — agent a's job ships the paths of agents 0 .. a - 1 as its context and gets what the searches before it
left of the budget — and mrp_ll_conflict_scan on their paths.  Every field is compared: status, cost, fmin, n_states,
expanded, tier, states, actions, action costs, planned, and the ten words of the conflict.

All roots run in ONE call per weight on an engine with four slots (more roots than slots); the expected answers are computed
in rounds, one batch of ordinary jobs per agent index over all roots.  Maps are 5 x 5 to 8 x 8, except the 64-agent root
(16 x 16) and the serpentine of the outgrown-table case (16 x 11), which needs paths of 65 states."""
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFLICT_KEYS = ("found", "time", "agent1", "agent2", "type", "x1", "y1", "x2", "y2", "count")
NO_NODE = dict(found=-1, time=0, agent1=0, agent2=0, type=0, x1=0, y1=0, x2=0, y2=0, count=0)
WS = (1.0, 1.5)


def _component(dimx, dimy, obstacles, seed_cell):
    obst = {tuple(o) for o in obstacles}
    seen, order = {tuple(seed_cell)}, [tuple(seed_cell)]
    for x, y in order:
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            c = (x + dx, y + dy)
            if 0 <= c[0] < dimx and 0 <= c[1] < dimy and c not in obst and c not in seen:
                seen.add(c)
                order.append(c)
    return order


def _random_map(dimx, dimy, n_obst, seed):
    rng = random.Random(seed)
    cells = [(x, y) for y in range(dimy) for x in range(dimx)]
    obst = rng.sample(cells, n_obst)
    free = [c for c in cells if c not in set(obst)]
    comp = max((_component(dimx, dimy, obst, c) for c in free[:8]), key=len)
    return dict(dimx=dimx, dimy=dimy, obstacles=[list(o) for o in obst]), sorted(comp)


def _snake(width, rows):
    """A serpentine corridor (even rows free, odd rows walls with one gap at alternating ends) and its cells in walking order."""
    obst, order = [], []
    for r in range(rows):
        xs = list(range(width)) if r % 2 == 0 else list(range(width - 1, -1, -1))
        order.extend((x, 2 * r) for x in xs)
        if r + 1 < rows:
            gap = xs[-1]
            order.append((gap, 2 * r + 1))
            obst.extend([x, 2 * r + 1] for x in range(width) if x != gap)
    return dict(dimx=width, dimy=2 * rows - 1, obstacles=obst), order


class _World:
    """Maps and heuristic tables of one engine, and roots by name."""

    def __init__(self, eng):
        self.eng, self.maps, self.roots, self.names, self._want = eng, {}, [], [], []

    def add(self, name, key, m, starts, goals, budget=-1):
        if key not in self.maps:
            self.maps[key] = self.eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        self.names.append(name)
        self.roots.append((key, [list(s) for s in starts], [None if g is None else list(g) for g in goals], budget))
        self._want.extend((key, tuple(g)) for g in goals if g is not None)

    def finish(self):
        from libmultirobotplanning_amd import ll
        want = sorted(set(self._want))
        ids = self.eng.compute_heuristics([self.maps[k] for k, _ in want], [list(g) for _, g in want])
        self.heur = dict(zip(want, ids))
        return [ll.TaRoot(map_id=self.maps[key], starts=starts, goals=goals,
                          heuristic_ids=[-1 if g is None else self.heur[(key, tuple(g))] for g in goals], max_expansions=budget)
                for key, starts, goals, budget in self.roots]


def _expected(eng, roots, w):
    """Per root [planned, [LLResult or None = not run], conflict dict, whole] from ordinary jobs, agent index by agent index."""
    from libmultirobotplanning_amd import ll
    got = [[] for _ in roots]
    left = [r.max_expansions for r in roots]
    alive = [True] * len(roots)
    for a in range(max(len(r.starts) for r in roots)):
        who = [i for i, r in enumerate(roots) if alive[i] and a < len(r.starts)]
        if not who:
            break
        jobs = []
        for i in who:
            r = roots[i]
            ctx = [[s[1:] for s in got[i][q].states] if q < a else [] for q in range(len(r.starts))]
            jobs.append(ll.LLJob(map_id=r.map_id, algo=ll.ASTAR_EPS_TA, start=r.starts[a], goal=r.goals[a], agent_idx=a, w=w,
                                 ctx_paths=ctx, max_expansions=left[i], heuristic_id=r.heuristic_ids[a]))
        for i, one in zip(who, eng.search_batch(jobs)):
            got[i].append(one)
            if one.status != ll.OK:
                alive[i] = False
            elif left[i] >= 0:
                left[i] = max(left[i] - one.expanded, 0)
    out, scans = [], []
    for i, r in enumerate(roots):
        whole = alive[i] and len(got[i]) == len(r.starts)
        if whole:
            scans.append((i, [[s[1:] for s in x.states] for x in got[i]]))
        out.append([len(got[i]), got[i] + [None] * (len(r.starts) - len(got[i])), dict(NO_NODE), whole])
    for (i, _), c in zip(scans, eng.conflict_scan([p for _, p in scans])):
        out[i][2] = c
    return out


def _same(name, got, exp):
    from libmultirobotplanning_amd import ll
    planned, row, conflict, _ = exp
    assert got.planned == planned, name
    assert len(got.results) == len(row), name
    for a, (g, e) in enumerate(zip(got.results, row)):
        if e is None:
            assert (g.status, g.cost, g.fmin, g.n_states, g.expanded, g.tier, g.states) == (ll.NOT_RUN, 0, 0, 0, 0, 0, []), (name, a)
            continue
        assert (g.status, g.cost, g.fmin, g.n_states, g.expanded, g.tier) == (e.status, e.cost, e.fmin, e.n_states, e.expanded, e.tier), (name, a, g, e)
        assert (g.states, g.actions, g.action_costs) == (e.states, e.actions, e.action_costs), (name, a)
    assert {k: got.conflict[k] for k in CONFLICT_KEYS} == {k: conflict[k] for k in CONFLICT_KEYS}, name


def _build_roots(w):
    # agent counts around the table's row padding (16) on 8 x 8, the limit on 16 x 16; some agents without a task
    m8, comp8 = _random_map(8, 8, 8, 3)
    for n in (1, 2, 16, 17):
        rng = random.Random(200 + n)
        starts, goals = rng.sample(comp8, n), rng.sample(comp8, n)
        w.add("n%d" % n, "m8", m8, starts, goals)
        w.add("n%d_idle" % n, "m8", m8, starts, [None if a % 4 == 1 else g for a, g in enumerate(goals)])
    m16, comp16 = _random_map(16, 16, 30, 5)
    rng = random.Random(264)
    w.add("n64", "m16", m16, rng.sample(comp16, 64), rng.sample(comp16, 64))
    # a taskless first agent: agent 1 searches against a one-row table
    open5 = dict(dimx=5, dimy=5, obstacles=[])
    w.add("idle_first", "open5", open5, [(2, 2), (0, 2), (2, 0)], [None, (4, 2), (2, 4)])
    # each path longer than all before it (the earlier columns are extended), then a short one; and the other way round
    open8 = dict(dimx=8, dimy=8, obstacles=[])
    w.add("growing", "open8", open8, [(0, 0), (0, 1), (0, 7), (3, 3)], [(1, 0), (4, 1), (7, 0), (3, 4)])
    w.add("shrinking", "open8", open8, [(0, 7), (0, 1), (0, 0), (3, 3)], [(7, 0), (4, 1), (1, 0), (3, 4)])
    # agents that cross: the later one sees the earlier one's path (w > 1 may walk around it), and the scan has something to count
    w.add("crossing", "open5", open5, [(0, 2), (2, 0), (4, 2)], [(4, 2), (2, 4), (0, 2)])
    line = dict(dimx=6, dimy=1, obstacles=[])
    w.add("swap", "line6", line, [(0, 0), (5, 0)], [(5, 0), (0, 0)])
    # a task that cannot be reached, in the middle: (4, 4) is walled in
    pocket = dict(dimx=6, dimy=6, obstacles=[[3, 4], [5, 4], [4, 3], [4, 5]])
    w.add("unreachable_mid", "pocket", pocket, [(0, 0), (1, 0), (2, 0)], [(2, 2), (4, 4), (5, 0)])
    w.add("probe", "m8", m8, comp8[:3], comp8[-3:])


@pytest.fixture(scope="module", params=WS)
def run(request):
    """(table name -> (root, result of ONE mrp_ll_ta_eps_root_batch call, expected), engine, world, w), four slots."""
    from libmultirobotplanning_amd import ll
    w = request.param
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=4)
    try:
        world = _World(eng)
        _build_roots(world)
        roots = world.finish()
        probe = _expected(eng, roots[-1:], w)[0]
        assert probe[3] and all(r.expanded >= 2 for r in probe[1])
        for name, budget in (("budget_mid", probe[1][0].expanded + probe[1][1].expanded - 1), ("budget_zero", probe[1][0].expanded)):
            world.names.append(name)
            roots.append(ll.TaRoot(map_id=roots[-1].map_id, starts=roots[-1].starts, goals=roots[-1].goals,
                                   heuristic_ids=roots[-1].heuristic_ids, max_expansions=budget))
        assert len(roots) > 4  # more roots than arena slots: a workgroup takes several
        got = eng.ta_eps_root_batch(roots, w)
        exp = _expected(eng, roots, w)
        yield dict(zip(world.names, zip(roots, got, exp))), eng, world, w
    finally:
        eng.close()


def _check(run, pick):
    table = run[0]
    names = [n for n in table if pick(n)]
    assert names
    for n in names:
        _same(n, table[n][1], table[n][2])
    return [table[n] for n in names]


def test_agent_counts_around_the_row_padding_and_at_the_limit(run):
    rows = _check(run, lambda n: n in ("n1", "n2", "n16", "n17", "n64"))
    assert sorted(len(r.starts) for r, _, _ in rows) == [1, 2, 16, 17, 64]
    assert all(g.planned == len(r.starts) and e[3] and g.conflict["found"] in (0, 1) for r, g, e in rows)
    assert all(x.tier == 1 for _, g, _ in rows for x in g.results)


def test_taskless_agents_and_a_taskless_first_agent(run):
    rows = _check(run, lambda n: n.endswith("_idle") or n == "idle_first")
    idle = [x for r, g, _ in rows for x, goal in zip(g.results, r.goals) if goal is None]
    assert idle and all(x.n_states == 1 and x.cost == 0 for x in idle)
    (_, first, _), = _check(run, lambda n: n == "idle_first")
    assert first.planned == 3 and first.results[0].n_states == 1


def test_a_path_longer_than_all_before_it_extends_the_table(run):
    (_, g, _), = _check(run, lambda n: n == "growing")
    lens = [x.n_states for x in g.results]
    assert lens[0] < lens[1] < lens[2] and lens[3] < lens[2]
    (_, s, _), = _check(run, lambda n: n == "shrinking")
    assert s.results[0].n_states > s.results[1].n_states > s.results[2].n_states


def test_later_agents_see_earlier_paths_and_the_count_is_the_focal_heuristic(run):
    (_, c, _), = _check(run, lambda n: n == "crossing")
    (_, s, e), = _check(run, lambda n: n == "swap")
    assert s.conflict["found"] == 1 and s.conflict["count"] == e[2]["count"] >= 1  # a corridor: nobody can walk around
    assert c.conflict["count"] >= 0 and c.planned == 3
    if run[3] == 1.0:  # fmin is the search's lower bound: at w = 1 the path's own cost
        assert all(x.fmin == x.cost for x in c.results)


def test_unreachable_task_in_the_middle_ends_the_root_behind_its_agent(run):
    from libmultirobotplanning_amd import ll
    (_, g, _), = _check(run, lambda n: n == "unreachable_mid")
    assert g.planned == 2 and g.conflict == NO_NODE
    assert g.results[0].status == ll.OK and g.results[1].status != ll.OK and g.results[2].status == ll.NOT_RUN


def test_budget_is_shared_across_the_root(run):
    from libmultirobotplanning_amd import ll
    (_, mid, _), = _check(run, lambda n: n == "budget_mid")
    assert [x.status for x in mid.results] == [ll.OK, ll.CAP_EXPANSIONS, ll.NOT_RUN] and mid.planned == 2 and mid.conflict == NO_NODE
    (_, zero, _), = _check(run, lambda n: n == "budget_zero")  # nothing left: the next search starts with 0
    assert [x.status for x in zero.results] == [ll.OK, ll.CAP_EXPANSIONS, ll.NOT_RUN] and zero.results[1].expanded == 1


def test_refused_root_between_two_good_ones_no_roots_and_busy(run):
    from libmultirobotplanning_amd import ll
    table, eng, _, w = run
    good = table["n2"][0]
    bad = [ll.TaRoot(map_id=999, starts=good.starts, goals=good.goals, heuristic_ids=good.heuristic_ids),
           ll.TaRoot(map_id=good.map_id, starts=[[8, 0], good.starts[1]], goals=good.goals, heuristic_ids=good.heuristic_ids),
           ll.TaRoot(map_id=good.map_id, starts=[good.starts[0]] * 65, goals=[None] * 65, heuristic_ids=[-1] * 65)]
    got = eng.ta_eps_root_batch([good, bad[0], table["crossing"][0], bad[1], bad[2], table["swap"][0]], w)
    for q, name in ((0, "n2"), (2, "crossing"), (5, "swap")):
        _same(name, got[q], table[name][2])
    for q in (1, 3, 4):
        assert got[q].planned == 0 and got[q].conflict == NO_NODE
        assert all((x.status, x.cost, x.fmin, x.n_states, x.expanded) == (ll.BAD_JOB, 0, 0, 0, 0) for x in got[q].results)
    assert eng.ta_eps_root_batch([], w) == []
    assert eng.ta_eps_root_batch([good], 0.5, raw_rc=True) == ll.E_INVALID
    eng.session_begin(4)
    try:
        assert eng.ta_eps_root_batch([good], w, raw_rc=True) == ll.E_BUSY
    finally:
        eng.session_end()
    _same("n2", eng.ta_eps_root_batch([good], w)[0], table["n2"][2])


def _outgrown_table_child():
    """Run in a fresh process under MRP_LL_ARENA_PATHS_BYTES=4096: 17 agents make rows of 32 cells, so a table of more than 64
    rows does not fit; the long paths have 63, 65 and 67 states.  long_last: the kernel stops behind agent 15 (65 states), the
    call runs agent 16 and scans; long_first: it stops behind agent 1, the call runs fifteen agents; long_last_budget: the
    budget runs out in the agent the call runs; three: rows of 16 cells, 67 rows fit, the device scans."""
    from libmultirobotplanning_amd import ll
    assert os.environ.get("MRP_LL_ARENA_PATHS_BYTES") == "4096"
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=2)
    try:
        world = _World(eng)
        snake, order = _snake(16, 6)
        long3 = [(order[0], order[62]), (order[10], order[74]), (order[20], order[86])]
        short = [(order[30 + 3 * a], order[32 + 3 * a]) for a in range(14)]
        world.add("three", "snake", snake, [p[0] for p in long3], [p[1] for p in long3])
        world.add("long_last", "snake", snake, [p[0] for p in short + long3], [p[1] for p in short + long3])
        world.add("long_first", "snake", snake, [p[0] for p in long3 + short], [p[1] for p in long3 + short])
        world.add("long_last_budget", "snake", snake, [p[0] for p in short + long3], [p[1] for p in short + long3])
        roots = world.finish()
        for w in WS:
            free = _expected(eng, roots[:3], w)
            spent = sum(x.expanded for x in free[1][1][:16])
            roots[3].max_expansions = spent + 5  # runs out in the part the call completes: in agent 16, the longest one
            got, exp = eng.ta_eps_root_batch(roots, w), free + _expected(eng, roots[3:], w)
            for name, g, e in zip(world.names, got, exp):
                _same(name, g, e)
            assert all(e[3] and g.conflict["found"] in (0, 1) for g, e in zip(got[:3], exp[:3]))
            assert max(x.n_states for x in got[1].results) >= 65 and got[1].planned == 17
            assert got[3].planned == 17 and got[3].results[16].status == ll.CAP_EXPANSIONS and got[3].conflict == NO_NODE
            assert [x.n_states for x in got[1].results[14:]] == [63, 65, 67]
    finally:
        eng.close()
    print("outgrown-table: ok")


def test_a_table_that_outgrows_the_path_area_is_finished_by_the_call():
    env = dict(os.environ, MRP_LL_ARENA_PATHS_BYTES="4096",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    run = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--outgrown-table"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0 and "outgrown-table: ok" in run.stdout, run.stdout[-4000:]


if __name__ == "__main__" and "--outgrown-table" in sys.argv:
    _outgrown_table_child()
