"""MRP_LL_JOB_TABLE_H on the MI355X: MRP_LL_ASTAR / MRP_LL_ASTAR_EPS searches whose h is the goal's shortest-path table
(csrc/ll_jobs.h runJobTableH over ll_arena_search.h's table form).  The yardstick is the CPU checker
(tests/support/table_h_check.cpp) over the cases of tests/table_h_cases.py, field by field: status, cost, fmin, expansion
count, states, actions."""
import pytest

import table_h_cases

pytestmark = pytest.mark.gpu


def _same_as_checker(r, o, tag):
    from libmultirobotplanning_amd import ll
    assert o["rc"] == 0, tag
    assert (r.success, r.expanded) == (o["success"], o["expanded"]), (tag, r.status, r.expanded, o["expanded"])
    if o["success"]:
        assert r.status == ll.OK, tag
        assert (r.cost, r.fmin, r.states, r.actions) == (o["cost"], o["fmin"], o["states"], o["actions"]), tag
        assert r.action_costs == [1] * len(o["actions"]), tag
    else:
        assert (r.status, r.states, r.n_states) == (ll.NO_SOLUTION, [], 0), tag


def _fields(r):
    return (r.status, r.success, r.cost, r.fmin, r.expanded, r.n_states, r.states, r.actions, r.action_costs, r.tier)


class _Bench:
    """One engine; maps by content; a case's table either uploaded from the host's BFS or computed on the device."""

    def __init__(self, computed, slots=64):
        from libmultirobotplanning_amd import ll
        self.ll = ll
        self.eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=slots)
        self.maps, self.heurs = {}, {}
        cases = table_h_cases.cases()
        for c in cases:
            m = c["map"]
            key = (m["dimx"], m["dimy"], tuple(map(tuple, m["obstacles"])))
            if key not in self.maps:
                self.maps[key] = self.eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
            c_map = self.maps[key]
            if (c_map, tuple(c["goal"])) not in self.heurs:
                self.heurs[(c_map, tuple(c["goal"]))] = None
        keys = list(self.heurs)
        if computed:
            ids = self.eng.compute_heuristics([k[0] for k in keys], [list(k[1]) for k in keys])
        else:
            by_key = {}
            for c in cases:
                by_key[(self.map_id(c["map"]), tuple(c["goal"]))] = c["table"]
            ids = [self.eng.upload_heuristic(k[0], by_key[k]) for k in keys]
        self.heurs = dict(zip(keys, ids))

    def close(self):
        self.eng.close()

    def map_id(self, m):
        return self.maps[(m["dimx"], m["dimy"], tuple(map(tuple, m["obstacles"])))]

    def job(self, algo, c, table_h=True):
        mid = self.map_id(c["map"])
        return self.ll.LLJob(map_id=mid, algo=self.ll.ASTAR_EPS if algo == 1 else self.ll.ASTAR, start=c["start"], goal=c["goal"],
                             agent_idx=c["agent"], w=c["w"], vertex_constraints=c["vc"], edge_constraints=c["ec"],
                             ctx_paths=c["ctx"] if algo == 1 else (), max_expansions=c["cap"],
                             initial_cost=c["initial_cost"] if algo == 0 else 0, table_h=table_h,
                             heuristic_id=self.heurs[(mid, tuple(c["goal"]))] if table_h else 0)


@pytest.fixture(scope="module")
def runs():
    return table_h_cases.runs()


@pytest.fixture(scope="module")
def batch_results(runs):
    """Every case in every algorithm through ONE mrp_ll_search_batch on computed tables, `wall` without the flag riding along."""
    b = _Bench(computed=True)
    try:
        wall = next(c for c in table_h_cases.cases() if c["name"] == "wall")
        jobs = [b.job(algo, c) for algo, c, _ in runs] + [b.job(algo, wall, table_h=False) for algo in (0, 1)]
        res = b.eng.search_batch(jobs)
        assert len(res) == len(jobs)
        return res
    finally:
        b.close()


def test_every_case_in_a_batch_equals_the_checker(runs, batch_results):
    for (algo, c, o), r in zip(runs, batch_results):
        tag = (c["name"], algo, r.status, r.tier)
        _same_as_checker(r, o, tag)
        if c["tier"] is not None:
            assert r.tier == c["tier"], tag
    by = {(c["name"], algo): r for (algo, c, _), r in zip(runs, batch_results)}
    from libmultirobotplanning_amd import ll
    assert (by[("unreachable", 0)].status, by[("unreachable", 0)].expanded) == (ll.NO_SOLUTION, 0)
    assert (by[("unreachable", 1)].status, by[("unreachable", 1)].expanded) == (ll.NO_SOLUTION, 0)
    assert by[("initial_cost", 0)].cost == by[("wall", 0)].cost + 7


def test_wall_without_the_flag_is_still_the_manhattan_search(runs, batch_results, oracle_mod):
    wall = next(c for c in table_h_cases.cases() if c["name"] == "wall")
    by = {(c["name"], algo): r for (algo, c, _), r in zip(runs, batch_results)}
    for algo, r in zip((0, 1), batch_results[len(runs):]):
        o = oracle_mod.ll_search(algo, wall["map"], 0, wall["start"], wall["goal"], w=wall["w"])
        assert (r.success, r.cost, r.fmin, r.expanded, r.states, r.actions) == (o["success"], o["cost"], o["fmin"], o["expanded"],
                                                                                o["states"], o["actions"]), algo
        assert by[("wall", algo)].expanded < r.expanded and by[("wall", algo)].cost == r.cost, algo


def test_uploaded_tables_and_a_mixed_session_give_the_same_answers(runs, batch_results):
    b = _Bench(computed=False)
    try:
        jobs = [b.job(algo, c) for algo, c, _ in runs]
        uploaded = b.eng.search_batch(jobs)
        b.eng.session_begin(16)
        try:
            session = b.eng.search_batch(jobs)
        finally:
            b.eng.session_end()
    finally:
        b.close()
    for (algo, c, _), ref, u, s in zip(runs, batch_results, uploaded, session):
        assert _fields(u) == _fields(ref), ("uploaded", c["name"], algo)
        assert _fields(s) == _fields(ref), ("session", c["name"], algo)


def test_a_one_algorithm_session_refuses_the_job_and_goes_on(runs, batch_results):
    from libmultirobotplanning_amd import ll
    wall = next(c for c in table_h_cases.cases() if c["name"] == "wall")
    b = _Bench(computed=True)
    try:
        for algo, session_algo in ((1, ll.ASTAR_EPS), (0, ll.ASTAR)):
            b.eng.session_begin_algo(session_algo, 8)
            try:
                flagged, plain = b.eng.search_batch([b.job(algo, wall), b.job(algo, wall, table_h=False)])
                again = b.eng.search_batch([b.job(algo, wall, table_h=False)])[0]
            finally:
                b.eng.session_end()
            assert (flagged.status, flagged.expanded, flagged.n_states) == (ll.BAD_JOB, 0, 0), algo
            assert plain.status == ll.OK and _fields(plain) == _fields(again), algo
            assert _fields(plain)[:9] == _fields(batch_results[len(runs) + (0 if algo == 0 else 1)])[:9], algo
    finally:
        b.close()


def test_refusals_come_back_as_bad_jobs(runs):
    """heuristic_id unknown or of another map, and the flag with a hint it does not combine with: MRP_LL_BAD_JOB for that job,
    the rest of the batch unaffected."""
    from libmultirobotplanning_amd import ll
    wall = next(c for c in table_h_cases.cases() if c["name"] == "wall")
    big = next(c for c in table_h_cases.cases() if c["name"] == "big")
    b = _Bench(computed=True)
    try:
        good = b.job(0, wall)
        unknown = b.job(1, wall)
        unknown.heuristic_id = 10 ** 6
        other_map = b.job(0, wall)
        other_map.heuristic_id = b.heurs[(b.map_id(big["map"]), tuple(big["goal"]))]
        heavy = b.job(1, wall)
        heavy.heavy = True
        res = b.eng.search_batch([good, unknown, other_map, heavy, good])
    finally:
        b.close()
    assert [r.status for r in res] == [ll.OK, ll.BAD_JOB, ll.BAD_JOB, ll.BAD_JOB, ll.OK]
    assert _fields(res[0]) == _fields(res[4])


# ---- the driver: mrp_hl_solve_batch_table_h ------------------------------------------------------------------------------
def _legal_schedule(inst, paths):
    obst = {tuple(o) for o in inst["obstacles"]}
    for a, p in enumerate(paths):
        assert p[0] == inst["starts"][a] and p[-1] == inst["goals"][a], a
        for (x0, y0), (x1, y1) in zip(p, p[1:]):
            assert abs(x1 - x0) + abs(y1 - y0) <= 1, a
        assert all(0 <= x < inst["dimx"] and 0 <= y < inst["dimy"] and (x, y) not in obst for x, y in p), a


def test_driver_on_the_reference_fixtures(ref_tests):
    from libmultirobotplanning_amd import hl
    names = ["mapf_simple1", "mapf_circle", "mapf_atGoal"]
    insts = [ref_tests["mapf"][n] for n in names]
    res, stats = hl.solve_batch_table_h(insts, algo=hl.CBS)
    assert [r["status"] for r in res] == [hl.SOLVED] * 3 and [r["cost"] for r in res] == [8, 4, 0]   # test/test_cbs.py:24-34
    assert [ref_tests["cbs_cost"][n] for n in names] == [8, 4, 0]
    assert stats["solved"] == 3 and stats["ll_expansions"] == sum(r["ll_expanded"] for r in res)
    res, _ = hl.solve_batch_table_h(insts, algo=hl.ECBS, w=1.0)
    assert [r["status"] for r in res] == [hl.SOLVED] * 3 and [r["cost"] for r in res] == [8, 4, 0]   # test/test_ecbs.py:25-35


def test_driver_on_sixteen_8x8_instances(oracle_mod):
    import numpy as np
    from libmultirobotplanning_amd import hl
    insts = table_h_cases.driver_instances()
    cap = table_h_cases.DRIVER_CAP
    solver = hl.BatchSolver(device=0, n_threads=2)
    try:
        man, _ = solver.solve(insts, algo=hl.CBS, max_ll_expansions=cap)
    finally:
        solver.close()
    assert [r["status"] for r in man] == [hl.SOLVED] * len(insts)
    cbs, st = hl.solve_batch_table_h(insts, algo=hl.CBS, max_ll_expansions=cap, n_threads=2)
    ecbs, _ = hl.solve_batch_table_h(insts, algo=hl.ECBS, w=1.3, max_ll_expansions=cap, n_threads=2)
    assert st["solved"] == len(insts)
    for k, (inst, m, c, e) in enumerate(zip(insts, man, cbs, ecbs)):
        assert c["status"] == hl.SOLVED and e["status"] == hl.SOLVED, k
        # CBS's sum of costs is the optimum under any admissible heuristic
        assert c["cost"] == m["cost"], (k, c["cost"], m["cost"])
        # the reference's bound: cost <= bestCost * w with the product in binary32 (ecbs.hpp focal bound)
        bound = np.float32(c["cost"]) * np.float32(1.3)
        assert isinstance(bound, np.float32) and np.float32(e["cost"]) <= bound, (k, e["cost"], c["cost"])
        for r in (c, e):
            _legal_schedule(inst, r["paths"])
            assert sum(len(p) - 1 for p in r["paths"]) == r["cost"], k
            assert oracle_mod.conflict_scan(r["paths"])["found"] == 0, k


def test_cli_ecbs_with_the_shortest_path_heuristic(ref_tests, tmp_path, capsys):
    import numpy as np
    import yaml
    from libmultirobotplanning_amd import cli
    inst = ref_tests["mapf"]["mapf_simple1"]
    inp, out = str(tmp_path / "in.yaml"), str(tmp_path / "out.yaml")
    with open(inp, "w") as f:
        yaml.safe_dump({"map": {"dimensions": [inst["dimx"], inst["dimy"]], "obstacles": inst["obstacles"]},
                        "agents": [{"name": "agent%d" % i, "start": s, "goal": g}
                                   for i, (s, g) in enumerate(zip(inst["starts"], inst["goals"]))]}, f)
    assert cli.main(["ecbs", "-i", inp, "-o", out, "-w", "1.3", "--heuristic", "shortest_path"]) == 0
    assert "Planning successful!" in capsys.readouterr().out
    doc = yaml.safe_load(open(out))
    assert list(doc["statistics"].keys()) == ["cost", "makespan", "runtime", "highLevelExpanded", "lowLevelExpanded"]
    sched = doc["schedule"]
    assert sorted(sched) == ["agent%d" % a for a in range(len(inst["starts"]))]
    paths = [[[s["x"], s["y"]] for s in sched["agent%d" % a]] for a in range(len(inst["starts"]))]
    assert all([s["t"] for s in sched["agent%d" % a]] == list(range(len(paths[a]))) for a in range(len(paths)))
    _legal_schedule(inst, paths)
    assert doc["statistics"]["cost"] == sum(len(p) - 1 for p in paths)
    assert np.float32(doc["statistics"]["cost"]) <= np.float32(8) * np.float32(1.3)  # (CBS's cost of the fixture is 8)
