"""mrp_ll_ta_root_batch on the MI355X: the root node of a CBS-TA conflict tree (cbs_ta.hpp:142-172) by one workgroup.

The yardstick is what the engine offers for the same work without the call, with the oracle behind it
(tests/test_ta_parity_gpu.py, tests/test_conflict_scan_gpu.py): the same agents as ordinary MRP_LL_ASTAR_TA jobs of
mrp_ll_search_batch, and mrp_ll_conflict_scan on their paths.  Every field is compared: status, cost, fmin, n_states,
expanded, tier, states, actions, action costs, planned, and the ten words of the conflict.

All roots run in ONE call on an engine with four slots (more roots than slots: a workgroup takes several); the expected
answers come from one batch of ordinary jobs, plus one small batch per agent for the two roots with a budget."""
import os
import random

import pytest

pytestmark = pytest.mark.gpu

CONFLICT_KEYS = ("found", "time", "agent1", "agent2", "type", "x1", "y1", "x2", "y2", "count")
NO_NODE = dict(found=-1, time=0, agent1=0, agent2=0, type=0, x1=0, y1=0, x2=0, y2=0, count=0)


def _component(dimx, dimy, obstacles, seed_cell):
    """The free cells connected to seed_cell, in BFS order."""
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
    """A serpentine corridor: the even rows are free, an odd row is a wall with one gap at alternating ends.  Returns the map
    and the corridor's cells in walking order: the only simple path between two of them runs along it."""
    dimy = 2 * rows - 1
    obst, order = [], []
    for r in range(rows):
        xs = list(range(width)) if r % 2 == 0 else list(range(width - 1, -1, -1))
        order.extend((x, 2 * r) for x in xs)
        if r + 1 < rows:
            gap = xs[-1]
            order.append((gap, 2 * r + 1))
            obst.extend([x, 2 * r + 1] for x in range(width) if x != gap)
    return dict(dimx=width, dimy=dimy, obstacles=obst), order


class _World:
    """Maps and heuristic tables of one engine, and roots by name."""

    def __init__(self, eng):
        self.eng, self.maps, self.roots, self.names = eng, {}, [], []
        self._want = []  # (map key, goal) of the tables to compute

    def map_id(self, key, m):
        if key not in self.maps:
            self.maps[key] = self.eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        return self.maps[key]

    def add(self, name, key, m, starts, goals, budget=-1):
        self.map_id(key, m)
        self.names.append(name)
        self.roots.append((key, [list(s) for s in starts], [None if g is None else list(g) for g in goals], budget))
        self._want.extend((key, tuple(g)) for g in goals if g is not None)

    def finish(self):
        """One mrp_ll_compute_heuristics launch for every goal; returns the ll.TaRoot list."""
        from libmultirobotplanning_amd import ll
        want = sorted(set(self._want))
        ids = self.eng.compute_heuristics([self.maps[k] for k, _ in want], [list(g) for _, g in want])
        self.heur = dict(zip(want, ids))
        out = []
        for key, starts, goals, budget in self.roots:
            hids = [-1 if g is None else self.heur[(key, tuple(g))] for g in goals]
            out.append(ll.TaRoot(map_id=self.maps[key], starts=starts, goals=goals, heuristic_ids=hids, max_expansions=budget))
        return out


def _jobs_of(root, caps):
    from libmultirobotplanning_amd import ll
    return [ll.LLJob(map_id=root.map_id, algo=ll.ASTAR_TA, start=s, goal=g, heuristic_id=h, max_expansions=c)
            for s, g, h, c in zip(root.starts, root.goals, root.heuristic_ids, caps)]


def _expected(eng, roots):
    """Per root (planned, [LLResult or None = not run], conflict dict) from ordinary jobs and mrp_ll_conflict_scan."""
    from libmultirobotplanning_amd import ll
    free = [i for i, r in enumerate(roots) if r.max_expansions < 0]
    jobs, where = [], []
    for i in free:
        js = _jobs_of(roots[i], [-1] * len(roots[i].starts))
        where.append((i, len(jobs), len(js)))
        jobs.extend(js)
    res = eng.search_batch(jobs)
    per_root = {i: res[o:o + n] for i, o, n in where}
    for i, r in enumerate(roots):  # a budget: each search gets what the ones before it left
        if r.max_expansions < 0:
            continue
        left, got = r.max_expansions, []
        for a in range(len(r.starts)):
            one = eng.search_batch(_jobs_of(r, [left] * len(r.starts))[a:a + 1])[0]
            got.append(one)
            if one.status != ll.OK:
                break
            left = max(left - one.expanded, 0)
        per_root[i] = got
    out, scans = [], []
    for i, r in enumerate(roots):
        got = list(per_root[i])
        bad = next((a for a, x in enumerate(got) if x.status != ll.OK), None)
        planned = len(got) if bad is None else bad + 1
        row = got[:planned] + [None] * (len(r.starts) - planned)
        whole = bad is None and planned == len(r.starts)
        if whole:
            scans.append((i, [[s[1:] for s in x.states] for x in got]))
        out.append([planned, row, dict(NO_NODE), whole])
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


def _build_roots(w, ref_tests):
    from test_oracle_known_answers import _ta_assignments
    # the three reference inputs under every assignment
    for name, inst in sorted(ref_tests["cbs_ta"]["inputs"].items()):
        m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
        for q, tasks in enumerate(_ta_assignments(inst["potential_goals"])):
            w.add("%s/%d" % (name, q), name, m, inst["starts"], tasks)
    # agent counts around the table's row padding (16) and at the limit, on a 32 x 32 map; every fifth agent has no task
    m32, comp = _random_map(32, 32, 120, 7)
    for n in (1, 2, 15, 16, 17, 64):
        rng = random.Random(100 + n)
        starts, goals = rng.sample(comp, n), rng.sample(comp, n)
        w.add("n%d" % n, "m32", m32, starts, goals)
        w.add("n%d_idle" % n, "m32", m32, starts, [None if a % 5 == 1 else g for a, g in enumerate(goals)])
    # two agents planned into a vertex conflict (they cross at (2, 2) at t = 2), two into an edge swap in a corridor
    open5 = dict(dimx=5, dimy=5, obstacles=[])
    w.add("vertex", "open5", open5, [(0, 2), (2, 0)], [(4, 2), (2, 4)])
    line4 = dict(dimx=4, dimy=1, obstacles=[])
    w.add("swap", "line4", line4, [(0, 0), (3, 0)], [(3, 0), (0, 0)])
    # a task that cannot be reached, at agent 0, in the middle and last: (4, 4) is walled in
    pocket = dict(dimx=6, dimy=6, obstacles=[[3, 4], [5, 4], [4, 3], [4, 5]])
    ok = [((0, 0), (2, 2)), ((1, 0), (0, 3)), ((2, 0), (5, 0))]
    for at in (0, 1, 2):
        pairs = list(ok)
        pairs[at] = (ok[at][0], (4, 4))
        w.add("unreachable%d" % at, "pocket", pocket, [p[0] for p in pairs], [p[1] for p in pairs])
    # paths of 63, 64 and 65 states along a serpentine: across the LDS tier's edge and past 64 table rows
    snake, order = _snake(16, 6)
    long3 = [(order[0], order[62]), (order[10], order[73]), (order[20], order[84])]
    w.add("snake", "snake", snake, [p[0] for p in long3], [p[1] for p in long3])
    # ... and with fourteen short ones: rows of 32 agents, a table of 65 x 64 bytes
    short = [(order[30 + a], order[33 + a]) for a in range(14)]
    w.add("snake17", "snake", snake, [p[0] for p in long3 + short], [p[1] for p in long3 + short])
    # a 40 x 40 map: the arena tier, tables of [dimy][dimx]
    m40, comp40 = _random_map(40, 40, 160, 11)
    rng = random.Random(40)
    w.add("m40", "m40", m40, rng.sample(comp40, 5), rng.sample(comp40, 4) + [None])
    return m32, comp


@pytest.fixture(scope="module")
def run(ref_tests):
    """(names, roots, results of ONE mrp_ll_ta_root_batch call, expected) on an engine with four slots."""
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=4)
    try:
        w = _World(eng)
        m32, comp = _build_roots(w, ref_tests)
        # a budget that runs out in the second of three searches, and one that is used up exactly by the first
        rng = random.Random(5)
        starts, goals = rng.sample(comp, 3), rng.sample(comp, 3)
        w.add("probe", "m32", m32, starts, goals)
        roots = w.finish()
        probe = eng.search_batch(_jobs_of(roots[-1], [-1, -1, -1]))
        assert all(r.status == ll.OK and r.expanded >= 2 for r in probe)
        for name, budget in (("budget_mid", probe[0].expanded + probe[1].expanded - 1), ("budget_zero", probe[0].expanded)):
            w.names.append(name)
            roots.append(ll.TaRoot(map_id=roots[-1].map_id, starts=starts, goals=goals, heuristic_ids=roots[-1].heuristic_ids,
                                   max_expansions=budget))
        assert len(roots) > 4  # more roots than slots
        got = eng.ta_root_batch(roots)
        exp = _expected(eng, roots)
        yield dict(zip(w.names, zip(roots, got, exp))), eng, w
    finally:
        eng.close()


def _check(run, pick):
    table = run[0]
    names = [n for n in table if pick(n)]
    assert names
    for n in names:
        _same(n, table[n][1], table[n][2])
    return [table[n] for n in names]


def test_reference_inputs_under_every_assignment(run):
    rows = _check(run, lambda n: n.startswith("mapfta_"))
    assert len(rows) == 4 and all(e[3] for _, _, e in rows)  # two assignments, one, one; every agent planned, every root scanned


def test_agent_counts_around_the_row_padding_and_at_the_limit(run):
    rows = _check(run, lambda n: n.startswith("n") and not n.endswith("_idle"))
    assert sorted(len(r.starts) for r, _, _ in rows) == [1, 2, 15, 16, 17, 64]
    assert all(g.planned == len(r.starts) for r, g, _ in rows)
    assert rows[0][1].conflict["found"] in (0, 1)


def test_agents_without_a_task_mixed_with_tasked_ones(run):
    rows = _check(run, lambda n: n.endswith("_idle"))
    idle = [x for r, g, _ in rows for x, goal in zip(g.results, r.goals) if goal is None]
    assert idle and all(x.n_states == 1 and x.cost == 0 for x in idle)  # a one-state path


def test_vertex_conflict_and_edge_swap(run):
    (_, v, _), = _check(run, lambda n: n == "vertex")
    assert (v.conflict["found"], v.conflict["type"], v.conflict["time"], v.conflict["x1"], v.conflict["y1"]) == (1, 0, 2, 2, 2)
    (_, s, _), = _check(run, lambda n: n == "swap")
    assert (s.conflict["found"], s.conflict["type"], s.conflict["time"]) == (1, 1, 1)


def test_unreachable_task_ends_the_root_behind_its_agent(run):
    from libmultirobotplanning_amd import ll
    rows = _check(run, lambda n: n.startswith("unreachable"))
    for at, (_, g, _) in enumerate(rows):
        assert g.planned == at + 1 and g.conflict == NO_NODE
        # The status is the ordinary job's, which _check has compared; on this engine that is CAP_HORIZON, not NO_SOLUTION:
        # the table says "no path" at the start cell, and both tiers answer that before the first pop (ll_compact.h
        # compactSearchTA "h0 > 254", ll_ta.h TaEnv::startH -> ST_CAP_HORIZON).  An unconstrained search of this Environment
        # cannot end NO_SOLUTION at all: a Wait is always a valid successor, so its open list never runs empty.
        assert [x.status for x in g.results[:at + 1]] == [ll.OK] * at + [ll.CAP_HORIZON]
        assert all(x.status == ll.NOT_RUN for x in g.results[at + 1:])


def test_budget_is_shared_like_a_root_chains(run):
    from libmultirobotplanning_amd import ll
    (_, mid, _), = _check(run, lambda n: n == "budget_mid")
    assert [x.status for x in mid.results] == [ll.OK, ll.CAP_EXPANSIONS, ll.NOT_RUN] and mid.planned == 2
    (_, zero, _), = _check(run, lambda n: n == "budget_zero")  # nothing left: the next search starts with 0
    assert [x.status for x in zero.results] == [ll.OK, ll.CAP_EXPANSIONS, ll.NOT_RUN]
    assert zero.results[1].expanded == 1 and zero.conflict == NO_NODE


def test_paths_across_the_lds_tiers_edge_and_past_64_rows(run):
    (_, g, _), = _check(run, lambda n: n == "snake")
    assert [x.n_states for x in g.results] == [63, 64, 65]
    assert [x.tier for x in g.results] == [0, 1, 1]
    _check(run, lambda n: n == "snake17")


def test_large_map_runs_in_the_arena_tier(run):
    (_, g, _), = _check(run, lambda n: n == "m40")
    assert all(x.tier == 1 for x in g.results[:4]) and g.planned == 5


def test_refused_roots_among_good_ones(run):
    from libmultirobotplanning_amd import ll
    table, eng, w = run
    good = table["n2"][0]
    other = w.heur[("snake", min(g for k, g in w.heur if k == "snake"))]
    bad = [ll.TaRoot(map_id=999, starts=good.starts, goals=good.goals, heuristic_ids=good.heuristic_ids),
           ll.TaRoot(map_id=good.map_id, starts=[[32, 0], good.starts[1]], goals=good.goals, heuristic_ids=good.heuristic_ids),
           ll.TaRoot(map_id=good.map_id, starts=good.starts, goals=good.goals, heuristic_ids=[good.heuristic_ids[0], other]),
           ll.TaRoot(map_id=good.map_id, starts=[], goals=[], heuristic_ids=[]),
           ll.TaRoot(map_id=good.map_id, starts=[good.starts[0]] * 65, goals=[None] * 65, heuristic_ids=[-1] * 65)]
    mixed = [good, bad[0], table["vertex"][0], bad[1], bad[2], bad[3], bad[4], table["swap"][0]]
    got = eng.ta_root_batch(mixed)
    for q, name in ((0, "n2"), (2, "vertex"), (7, "swap")):
        _same(name, got[q], table[name][2])
    for q in (1, 3, 4, 5, 6):
        assert got[q].planned == 0 and got[q].conflict == NO_NODE
        assert all((x.status, x.cost, x.fmin, x.n_states, x.expanded) == (ll.BAD_JOB, 0, 0, 0, 0) for x in got[q].results)
    assert eng.ta_root_batch([]) == []


def test_busy_inside_a_session_and_while_a_batch_is_in_flight(run):
    from libmultirobotplanning_amd import ll
    table, eng, _ = run
    handle = eng.submit_sets(_jobs_of(table["n2"][0], [-1, -1]))  # submitted, not waited for
    try:
        assert eng.ta_root_batch([table["vertex"][0]], raw_rc=True) == ll.E_BUSY
    finally:
        eng.wait_sets(handle, want_conflicts=False)
    eng.session_begin(4)
    try:
        assert eng.ta_root_batch([table["vertex"][0]], raw_rc=True) == ll.E_BUSY
    finally:
        eng.session_end()
    _same("vertex", eng.ta_root_batch([table["vertex"][0]])[0], table["vertex"][2])


def test_host_completes_the_scan_when_the_table_does_not_fit(ref_tests):
    """A context whose path area holds 4096 bytes: snake17's table (65 rows of 32 agents) does not fit, the three-agent
    one (65 rows of 16) does.  Same answers either way."""
    from libmultirobotplanning_amd import ll
    old = os.environ.get("MRP_LL_ARENA_PATHS_BYTES")
    os.environ["MRP_LL_ARENA_PATHS_BYTES"] = "4096"
    try:
        eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=2)
    finally:
        if old is None:
            del os.environ["MRP_LL_ARENA_PATHS_BYTES"]
        else:
            os.environ["MRP_LL_ARENA_PATHS_BYTES"] = old
    try:
        w = _World(eng)
        snake, order = _snake(16, 6)
        long3 = [(order[0], order[62]), (order[10], order[73]), (order[20], order[84])]
        short = [(order[30 + a], order[33 + a]) for a in range(14)]
        w.add("snake", "snake", snake, [p[0] for p in long3], [p[1] for p in long3])
        w.add("snake17", "snake", snake, [p[0] for p in long3 + short], [p[1] for p in long3 + short])
        w.add("snake17b", "snake", snake, [p[0] for p in short + long3], [p[1] for p in short + long3])
        roots = w.finish()
        got, exp = eng.ta_root_batch(roots), _expected(eng, roots)
        for name, g, e in zip(w.names, got, exp):
            _same(name, g, e)
            assert e[3] and g.conflict["found"] in (0, 1)
        assert got[1].conflict["count"] > 0  # the short paths overlap: the completed scan has something to say
    finally:
        eng.close()
