"""mrp_ll_ta_eps_root_batch_w on the MI355X: the root node of an ECBS-TA conflict tree of up to 256 agents by one workgroup,
with ONE table of up to 256 columns in the arena slot as the next search's focal context and as the scan's input.

The yardstick is tests/test_ta_eps_root_gpu.py's, whose helpers are used as they are: the same agents as ordinary
MRP_LL_ASTAR_EPS_TA jobs run one after another — agent a's job ships the paths of agents 0 .. a - 1 as its context and gets
what the searches before it left of the budget — and mrp_ll_conflict_scan on their paths.  Every field is compared.

The roots are tests/test_ta_root_wide_gpu.py's (agent counts on both sides of every group of 64 columns, conflicts, long
paths and failure points in groups other than 0).  All roots run in ONE call per weight on an engine with four slots; the
expected answers are computed in rounds, one batch of ordinary jobs per agent index over all roots."""
import pytest

from test_ta_eps_root_gpu import NO_NODE, _World, _expected, _same
from test_ta_root_wide_gpu import COUNTS, add_budget_root, build_roots, outgrown_roots, small_path_area_engine

pytestmark = pytest.mark.gpu

WS = (1.0, 1.3)


@pytest.fixture(scope="module", params=WS)
def run(request):
    """(name -> (root, result of ONE mrp_ll_ta_eps_root_batch_w call, expected), engine, world, w, budget agent), four slots."""
    from libmultirobotplanning_amd import ll
    w = request.param
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=4)
    try:
        world = _World(eng)
        build_roots(world)
        roots = world.finish()
        exp = _expected(eng, roots, w)
        probe = exp[world.names.index("n80")]
        assert probe[3]
        at = add_budget_root(world, roots, [r.expanded for r in probe[1]])
        exp += _expected(eng, roots[-1:], w)
        got = eng.ta_eps_root_batch(roots, w, wide=True)
        yield dict(zip(world.names, zip(roots, got, exp))), eng, world, w, at
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
    assert all(x.tier == 1 for _, g, _ in rows for x in g.results)
    idle = [x for r, g, _ in rows for x, goal in zip(g.results, r.goals) if goal is None]
    assert idle and all(x.n_states == 1 and x.cost == 0 for x in idle)


def test_roots_of_at_most_64_agents_equal_the_narrow_call(run):
    table, eng, _, w, _ = run
    narrow = eng.ta_eps_root_batch([table["n1"][0], table["n64"][0]], w)
    for name, g in zip(("n1", "n64"), narrow):
        _same(name, g, table[name][2])
        wide = table[name][1]
        assert (g.planned, g.conflict) == (wide.planned, wide.conflict)
        assert [(x.status, x.cost, x.fmin, x.n_states, x.expanded, x.tier, x.states) for x in g.results] == \
               [(x.status, x.cost, x.fmin, x.n_states, x.expanded, x.tier, x.states) for x in wide.results]


def test_conflicts_across_groups(run):
    (_, v, _), = _check(run, lambda n: n == "vertex_3_200")
    (_, s, _), = _check(run, lambda n: n == "swap_64_65")
    (_, t, _), = _check(run, lambda n: n == "two_conflicts")
    c = s.conflict  # a corridor: nobody can walk around, whatever the weight
    assert (c["found"], c["type"], c["agent1"], c["agent2"]) == (1, 1, 64, 65) and c["count"] >= 1
    if run[3] == 1.0:  # the shortest paths: the crossings of tests/test_ta_root_wide_gpu.py
        assert (v.conflict["found"], v.conflict["time"], v.conflict["agent1"], v.conflict["agent2"]) == (1, 2, 3, 200)
        assert (t.conflict["found"], t.conflict["time"], t.conflict["agent1"], t.conflict["agent2"]) == (1, 2, 130, 200)


def test_a_later_longer_path_extends_the_rows_in_all_groups(run):
    (_, g, _), = _check(run, lambda n: n == "snake141")
    lens = [x.n_states for x in g.results]
    assert lens[70] >= 63 and lens[140] >= 65 and lens[140] > lens[70] > max(lens[:70] + lens[71:140]) and g.planned == 141


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
    at = run[4]
    assert 64 <= at < 128 and g.planned == at + 1 and g.conflict == NO_NODE
    assert g.results[at].status == ll.CAP_EXPANSIONS and all(x.status == ll.NOT_RUN for x in g.results[at + 1:])


def test_refused_root_between_two_good_ones_and_the_stored_variant(run):
    from libmultirobotplanning_amd import ll
    table, eng, _, w, _ = run
    good = table["n65"][0]
    bad = ll.TaRoot(map_id=good.map_id, starts=[good.starts[0]] * 257, goals=[None] * 257, heuristic_ids=[-1] * 257)
    got = eng.ta_eps_root_batch([good, bad, table["swap_64_65"][0]], w, wide=True)
    _same("n65", got[0], table["n65"][2])
    _same("swap_64_65", got[2], table["swap_64_65"][2])
    assert got[1].planned == 0 and got[1].conflict == NO_NODE and len(got[1].results) == 257
    assert all((x.status, x.cost, x.fmin, x.n_states, x.expanded) == (ll.BAD_JOB, 0, 0, 0, 0) for x in got[1].results)
    narrow = eng.ta_eps_root_batch([good], w)[0]  # the narrow call still refuses what the wide one takes
    assert narrow.planned == 0 and all(x.status == ll.BAD_JOB for x in narrow.results)
    with pytest.raises(ValueError):
        eng.ta_eps_root_batch([table["n1"][0]], w, result_path_ids=[[-1]], wide=True)
    assert eng.ta_eps_root_batch([], w, wide=True) == []
    assert eng.ta_eps_root_batch([good], 0.5, raw_rc=True, wide=True) == ll.E_INVALID
    eng.session_begin(4)
    try:
        assert eng.ta_eps_root_batch([good], w, raw_rc=True, wide=True) == ll.E_BUSY
    finally:
        eng.session_end()


@pytest.mark.parametrize("w", WS)
def test_a_table_that_outgrows_the_path_area_is_finished_by_the_call(w):
    """Rows of 80 columns, 25 rows fit: the kernel stops behind the agent with 30 states — agent 40: the call plans 24 more
    agents with shipped contexts of 65 columns; agent 64: it only scans; agent 0: it plans all the others."""
    eng = small_path_area_engine()
    try:
        world = _World(eng)
        outgrown_roots(world)
        roots = world.finish()
        got, exp = eng.ta_eps_root_batch(roots, w, wide=True), _expected(eng, roots, w)
        for name, g, e in zip(world.names, got, exp):
            _same(name, g, e)
            assert e[3] and g.planned == 65 and g.conflict["found"] in (0, 1)
        assert all(max(x.n_states for x in g.results) >= 30 for g in got[:3])
    finally:
        eng.close()
