"""mrp_ll_ta_root_batch_w on the MI355X: the root node of a CBS-TA conflict tree of up to 256 agents by one workgroup.

The yardstick is tests/test_ta_root_gpu.py's, whose helpers are used as they are: the same agents as ordinary
MRP_LL_ASTAR_TA jobs of mrp_ll_search_batch, and mrp_ll_conflict_scan on their paths.  Every field is compared.

All roots run in ONE call on an engine with four slots.  What the shapes are for: lane l of the workgroup keeps agents
l + 64 k, k < 4, so the agent counts stand on both sides of every group's edge and of the row padding (16) inside a group;
the conflicts, the long paths and the failure points lie in groups other than 0.  Idle agents (no task: a one-state path)
fill the indices in between; they stand in rows nobody walks through."""
import os
import random

import pytest

from test_ta_root_gpu import NO_NODE, _World, _expected, _jobs_of, _random_map, _same, _snake

pytestmark = pytest.mark.gpu

COUNTS = (1, 64, 65, 80, 81, 128, 129, 193, 256)


def idle_cells(n, first_row, dimx=32):
    """n cells, row by row from first_row: where the agents without a task stand."""
    return [(q % dimx, first_row + q // dimx) for q in range(n)]


def filled(n, actors, first_row=20):
    """starts, goals of an n-agent root: actors = {agent: (start, goal)}, every other agent idle on a cell of its own."""
    cells = iter(idle_cells(n, first_row))
    starts, goals = [], []
    for a in range(n):
        s, g = actors[a] if a in actors else (next(cells), None)
        starts.append(s)
        goals.append(g)
    return starts, goals


def pocket32():
    """An open 32 x 32 map whose cell (30, 2) is walled in."""
    return dict(dimx=32, dimy=32, obstacles=[[29, 2], [31, 2], [30, 1], [30, 3]])


def swap_map():
    """Row 0: a corridor of six cells; row 1: a wall; rows 2 and 3: free, for the idle agents."""
    return dict(dimx=32, dimy=4, obstacles=[[x, 0] for x in range(6, 32)] + [[x, 1] for x in range(32)])


def build_roots(w):
    """The roots every wide root test uses (tests/test_ta_eps_root_wide_gpu.py too).  Returns (m32, comp)."""
    m32, comp = _random_map(32, 32, 100, 17)
    for n in COUNTS:  # every fifth agent has no task
        rng = random.Random(300 + n)
        starts = rng.sample(comp, n)
        goals = [None if a % 5 == 1 else rng.choice(comp[max(0, comp.index(tuple(s)) - 40):][:80]) for a, s in enumerate(starts)]
        w.add("n%d" % n, "m32", m32, starts, goals)
    open32 = dict(dimx=32, dimy=32, obstacles=[])
    # a vertex conflict between agents 3 and 200: they cross at (2, 2) at t = 2
    w.add("vertex_3_200", "open32", open32, *filled(201, {3: ((0, 2), (4, 2)), 200: ((2, 0), (2, 4))}))
    # an edge swap between agents 64 and 65 in a corridor
    w.add("swap_64_65", "swap", swap_map(), *filled(66, {64: ((0, 0), (5, 0)), 65: ((5, 0), (0, 0))}, first_row=2))
    # two conflicts: agents 0 and 1 cross at (10, 10) at t = 6, agents 130 and 200 at (2, 2) at t = 2 — the earlier one
    w.add("two_conflicts", "open32", open32, *filled(201, {0: ((4, 10), (16, 10)), 1: ((10, 4), (10, 16)),
                                                          130: ((0, 2), (4, 2)), 200: ((2, 0), (2, 4))}))
    # the longest paths in groups 1 and 2: 63 states at agent 70, 65 at agent 140 along a serpentine, the rest three states
    snake, order = _snake(32, 6)
    actors = {a: (order[40 + a], order[42 + a]) for a in range(141)}
    actors[70], actors[140] = (order[0], order[62]), (order[10], order[74])
    w.add("snake141", "snake32", snake, *filled(141, actors))
    # a task that cannot be reached at agent 64, 130 and 255: the last one a group holds, one inside, the very last
    for at, n in ((64, 66), (130, 132), (255, 256)):
        actors = {a: ((a % 28, 5 + a // 28), (a % 28, 6 + a // 28)) for a in range(0, n, 3)}  # every third walks one step
        actors[at] = ((0, 0), (30, 2))
        w.add("unreachable%d" % at, "pocket32", pocket32(), *filled(n, actors))
    return m32, comp


def add_budget_root(w, roots, probe_expanded):
    """n80 again with a budget that runs out in agent 70's search (group 1)."""
    from libmultirobotplanning_amd import ll
    src = roots[w.names.index("n80")]
    at = next(a for a in range(66, 80) if src.goals[a] is not None and probe_expanded[a] >= 2)
    w.names.append("budget_group1")
    roots.append(ll.TaRoot(map_id=src.map_id, starts=src.starts, goals=src.goals, heuristic_ids=src.heuristic_ids,
                           max_expansions=sum(probe_expanded[:at + 1]) - 1))
    return at


@pytest.fixture(scope="module")
def run():
    """(name -> (root, result of ONE mrp_ll_ta_root_batch_w call, expected), engine, world) on an engine with four slots."""
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=4)
    try:
        w = _World(eng)
        build_roots(w)
        roots = w.finish()
        probe = eng.search_batch(_jobs_of(roots[w.names.index("n80")], [-1] * 80))
        at = add_budget_root(w, roots, [r.expanded for r in probe])
        got = eng.ta_root_batch(roots, wide=True)
        exp = _expected(eng, roots)
        yield dict(zip(w.names, zip(roots, got, exp))), eng, w, at
    finally:
        eng.close()


def _check(run, pick):
    table = run[0]
    names = [n for n in table if pick(n)]
    assert names
    for n in names:
        _same(n, table[n][1], table[n][2])
    return [table[n] for n in names]


def test_agent_counts_on_both_sides_of_every_group(run):
    rows = _check(run, lambda n: n[1:].isdigit())
    assert tuple(len(r.starts) for r, _, _ in rows) == COUNTS
    assert all(g.planned == len(r.starts) and e[3] and g.conflict["found"] in (0, 1) for r, g, e in rows)
    idle = [x for r, g, _ in rows for x, goal in zip(g.results, r.goals) if goal is None]
    assert idle and all(x.n_states == 1 and x.cost == 0 for x in idle)


def test_roots_of_at_most_64_agents_equal_the_narrow_call(run):
    table, eng, _, _ = run
    narrow = eng.ta_root_batch([table["n1"][0], table["n64"][0]])
    for name, g in zip(("n1", "n64"), narrow):
        _same(name, g, table[name][2])
        wide = table[name][1]
        assert (g.planned, g.conflict) == (wide.planned, wide.conflict)
        assert [(x.status, x.cost, x.fmin, x.n_states, x.expanded, x.tier, x.states) for x in g.results] == \
               [(x.status, x.cost, x.fmin, x.n_states, x.expanded, x.tier, x.states) for x in wide.results]


def test_conflicts_across_groups(run):
    (_, v, _), = _check(run, lambda n: n == "vertex_3_200")
    c = v.conflict
    assert (c["found"], c["type"], c["time"], c["agent1"], c["agent2"], c["x1"], c["y1"]) == (1, 0, 2, 3, 200, 2, 2)
    (_, s, _), = _check(run, lambda n: n == "swap_64_65")
    c = s.conflict
    assert (c["found"], c["type"], c["time"], c["agent1"], c["agent2"]) == (1, 1, 2, 64, 65)
    (_, t, _), = _check(run, lambda n: n == "two_conflicts")
    c = t.conflict
    assert (c["found"], c["time"], c["agent1"], c["agent2"]) == (1, 2, 130, 200) and c["count"] >= 2


def test_longest_paths_in_groups_one_and_two(run):
    (_, g, _), = _check(run, lambda n: n == "snake141")
    lens = [x.n_states for x in g.results]
    assert (lens[70], lens[140]) == (63, 65) and max(lens[:70] + lens[71:140]) == 3 and g.planned == 141


def test_unreachable_task_ends_the_root_behind_its_agent(run):
    from libmultirobotplanning_amd import ll
    rows = _check(run, lambda n: n.startswith("unreachable"))
    for at, (r, g, _) in zip((64, 130, 255), rows):
        assert g.planned == at + 1 and g.conflict == NO_NODE
        assert all(x.status == ll.OK for x in g.results[:at]) and g.results[at].status not in (ll.OK, ll.NOT_RUN)
        assert all(x.status == ll.NOT_RUN for x in g.results[at + 1:]) and len(g.results) == len(r.starts)


def test_budget_runs_out_inside_group_one(run):
    from libmultirobotplanning_amd import ll
    (_, g, _), = _check(run, lambda n: n == "budget_group1")
    at = run[3]
    assert 64 <= at < 128 and g.planned == at + 1 and g.conflict == NO_NODE
    assert g.results[at].status == ll.CAP_EXPANSIONS and all(x.status == ll.NOT_RUN for x in g.results[at + 1:])


def test_refused_root_between_two_good_ones_and_busy(run):
    from libmultirobotplanning_amd import ll
    table, eng, _, _ = run
    good = table["n65"][0]
    bad = ll.TaRoot(map_id=good.map_id, starts=[good.starts[0]] * 257, goals=[None] * 257, heuristic_ids=[-1] * 257)
    got = eng.ta_root_batch([good, bad, table["swap_64_65"][0]], wide=True)
    _same("n65", got[0], table["n65"][2])
    _same("swap_64_65", got[2], table["swap_64_65"][2])
    assert got[1].planned == 0 and got[1].conflict == NO_NODE and len(got[1].results) == 257
    assert all((x.status, x.cost, x.fmin, x.n_states, x.expanded) == (ll.BAD_JOB, 0, 0, 0, 0) for x in got[1].results)
    # the narrow call still refuses what the wide one takes
    narrow = eng.ta_root_batch([good])[0]
    assert narrow.planned == 0 and all(x.status == ll.BAD_JOB for x in narrow.results)
    assert eng.ta_root_batch([], wide=True) == []
    eng.session_begin(4)
    try:
        assert eng.ta_root_batch([good], raw_rc=True, wide=True) == ll.E_BUSY
    finally:
        eng.session_end()


def small_path_area_engine():
    """An engine whose arena slots have a path area of 4096 bytes."""
    from libmultirobotplanning_amd import ll
    old = os.environ.get("MRP_LL_ARENA_PATHS_BYTES")
    os.environ["MRP_LL_ARENA_PATHS_BYTES"] = "4096"
    try:
        return ll.LowLevelEngine(device=0, n_tickets=1, slots=2)
    finally:
        if old is None:
            del os.environ["MRP_LL_ARENA_PATHS_BYTES"]
        else:
            os.environ["MRP_LL_ARENA_PATHS_BYTES"] = old


def outgrown_roots(w):
    """65 agents make rows of 80 columns: 25 rows fit 4096 bytes.  A path of 30 states at agent 40 (and at agent 64, and at
    agent 0) does not; fits: the longest path has 24 states."""
    open32 = dict(dimx=32, dimy=32, obstacles=[])
    short = {a: ((a % 30, 5 + 2 * (a // 30)), (a % 30 + 2, 5 + 2 * (a // 30))) for a in range(0, 65, 2)}
    for name, at, steps in (("long40", 40, 29), ("long64", 64, 29), ("long0", 0, 29), ("fits", 40, 23)):
        actors = dict(short)
        actors[at] = ((0, 0), (steps, 0))
        w.add(name, "open32", open32, *filled(65, actors))


def test_host_completes_the_scan_when_the_table_does_not_fit():
    eng = small_path_area_engine()
    try:
        w = _World(eng)
        outgrown_roots(w)
        roots = w.finish()
        got, exp = eng.ta_root_batch(roots, wide=True), _expected(eng, roots)
        for name, g, e in zip(w.names, got, exp):
            _same(name, g, e)
            assert e[3] and g.planned == 65 and g.conflict["found"] in (0, 1)
        assert [max(x.n_states for x in g.results) for g in got] == [30, 30, 30, 24]
    finally:
        eng.close()
