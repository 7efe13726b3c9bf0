"""Shortest-path heuristic tables computed on the MI355X (mrp_ll_compute_heuristics / mrp_ll_read_heuristic /
mrp_ll_heuristic_lookup): every table against a plain BFS (tests/heuristic_inputs.py), the task-assignment searches with
computed ids against the same searches with uploaded ids and against their oracles, persistence across growth of the
device buffer, the lookup, the error codes, the launch count and the CLI front-end.  All comparisons are exact."""
import ctypes
import itertools

import numpy as np
import pytest

import ecbs_ta_checker as checker
import ecbs_ta_corpus
import heuristic_inputs as hi

pytestmark = pytest.mark.gpu

E_INVALID, E_BUSY = -1, -4
I32P = ctypes.POINTER(ctypes.c_int32)


def _assignments(potential_goals):
    """Every assignment of distinct goals that gives a task to as many agents as possible (tiny fixtures: brute force)."""
    best, out = -1, []
    choices = [[None] + [tuple(g) for g in pg] for pg in potential_goals]
    for combo in itertools.product(*choices):
        used = [c for c in combo if c is not None]
        if len(set(used)) != len(used):
            continue
        if len(used) > best:
            best, out = len(used), []
        if len(used) == best:
            out.append([list(c) if c is not None else None for c in combo])
    return out


def _tables(eng, inputs):
    """ONE compute call for all (map, goal) pairs of `inputs`; returns [(map, goal, heuristic id)]."""
    mids, goals, rows = [], [], []
    for m, gs in inputs:
        mid = eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        for g in gs:
            mids.append(mid)
            goals.append(list(g))
            rows.append((m, g))
    hids = eng.compute_heuristics(mids, goals)
    assert len(hids) == len(rows) and len(set(hids)) == len(hids)
    return [(m, g, h) for (m, g), h in zip(rows, hids)]


def _check_tables(eng, rows):
    for m, g, h in rows:
        got = eng.read_heuristic(h)
        want = hi.bfs(m["dimx"], m["dimy"], m["obstacles"], g)
        assert got.shape == want.shape and np.array_equal(got, want), (m["dimx"], m["dimy"], g, np.argwhere(got != want)[:5].tolist())
    return len(rows)


def test_tables_equal_bfs_small_and_large_maps():
    """The inputs of the emulator test through the device, one compute call per map size class; read_heuristic of an
    uploaded table returns what was uploaded (values beyond the halfword range come back as unreachable)."""
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64, max_cells=65025)
    try:
        small = _tables(eng, hi.small_inputs())
        large = _tables(eng, hi.large_inputs())
        assert _check_tables(eng, small) >= 200
        assert _check_tables(eng, large) >= 30
        for m, g in ((hi.serpentine(), (0, 12)), (hi.random_map(48, 48, 101), (0, 47))):
            mid = eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
            up = hi.bfs(m["dimx"], m["dimy"], m["obstacles"], g)
            assert np.array_equal(eng.read_heuristic(eng.upload_heuristic(mid, up)), up)
            odd = (np.arange(m["dimx"] * m["dimy"], dtype=np.int64).reshape(m["dimy"], m["dimx"]) * 37) % 70000
            back = eng.read_heuristic(eng.upload_heuristic(mid, odd))
            assert np.array_equal(back, np.where(odd > 0xFFFE, hi.INF, odd))
        assert _check_tables(eng, small[:20] + large[:5]) == 25  # still there after the uploads behind them
    finally:
        eng.close()


# ---- searches: uploaded ids against computed ids ------------------------------------------------------------------

def _ta_cases(oracle_mod, ref_tests, bench_instances):
    """MRP_LL_ASTAR_TA cases (map, start, goal, vc, ec, cap, oracle) built as tests/test_ta_parity_gpu.py builds them: the
    reference's fixtures, random constraint sets, and searches beyond the LDS tier."""
    cases = []
    for name, inst in ref_tests["cbs_ta"]["inputs"].items():
        m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
        for tasks in _assignments(inst["potential_goals"]):
            _, calls = oracle_mod.ta_cbs_fixed(m, inst["starts"], tasks)
            for c in calls:
                cases.append((m, inst["starts"][c["agent"]], c["goal"], c["vertex_constraints"], c["edge_constraints"], -1))
    rng = np.random.default_rng(5)
    maps = {}
    for trial in range(120):
        name = "map_8by8_obst12_agents8_ex%d" % (trial % 5) if trial % 2 else "map_32by32_obst204_agents10_ex%d" % (trial % 7)
        inst = bench_instances[name]
        m = maps.setdefault(name, dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"]))
        d = inst["dimx"]
        a = int(rng.integers(0, len(inst["starts"])))
        goal = None if trial % 3 == 0 else inst["goals"][a]
        vc = [[int(rng.integers(0, 14)), int(rng.integers(0, d)), int(rng.integers(0, d))] for _ in range(int(rng.integers(0, 90)))]
        if goal is not None and trial % 4 == 1:
            vc.append([int(rng.integers(3, 20)), goal[0], goal[1]])
        ec = []
        for _ in range(int(rng.integers(0, 90))):
            x, y = int(rng.integers(0, d)), int(rng.integers(0, d))
            dx, dy = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)][int(rng.integers(0, 5))]
            ec.append([int(rng.integers(0, 14)), x, y, x + dx, y + dy])
        cases.append((m, inst["starts"][a], goal, vc, ec, int(rng.choice([-1, -1, -1, 25]))))
    # beyond the LDS tier (result.tier == 1): the 198-step serpentine, a goal constraint 150 steps out, a 48 x 48 map
    snake = hi.serpentine()
    inst = bench_instances["map_32by32_obst204_agents10_ex3"]
    m32 = maps.setdefault("map_32by32_obst204_agents10_ex3", dict(dimx=32, dimy=32, obstacles=inst["obstacles"]))
    m48 = hi.random_map(48, 48, 101, density=0.18)
    # start and goal inside one large free component: the reference never returns from a search for an unreachable goal
    for s48 in hi.free_cells(m48):
        from_start = hi.bfs(48, 48, m48["obstacles"], s48)
        if (from_start < hi.INF).sum() > 1500:
            break
    fy, fx = np.unravel_index(np.argmax(np.where(from_start < hi.INF, from_start, -1)), from_start.shape)
    far = [int(fx), int(fy)]
    assert from_start[fy, fx] > 62
    cases.append((snake, [0, 0], [0, 12], [], [], -1))
    cases.append((snake, [0, 0], [0, 12], [[230, 0, 12]], [[100, 12, 6, 13, 6]], -1))
    g = inst["goals"][2]
    cases.append((m32, inst["starts"][2], g, [[150, g[0], g[1]]], [], -1))
    cases.append((m48, s48, list(far), [], [], -1))
    return [c + (oracle_mod.ta_ll_search(c[0], c[1], c[2], c[3], c[4], cap_expansions=c[5], cap=1024),) for c in cases]


def _heuristic_ids(eng, pairs, computed, all_maps=()):
    """pairs: [(map dict, goal)] (distinct).  Uploads every map (those of `pairs` and `all_maps`) once; one table per pair,
    uploaded from the host BFS or computed on the device.  Returns ({id(map): map id}, {(id(map), goal): heuristic id})."""
    maps, heurs = {}, {}
    for m in [p[0] for p in pairs] + list(all_maps):
        if id(m) not in maps:
            maps[id(m)] = eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
    if computed:
        hids = eng.compute_heuristics([maps[id(m)] for m, _ in pairs], [list(g) for _, g in pairs])
        for (m, g), h in zip(pairs, hids):
            heurs[(id(m), tuple(g))] = h
    else:
        for m, g in pairs:
            heurs[(id(m), tuple(g))] = eng.upload_heuristic(maps[id(m)], hi.bfs(m["dimx"], m["dimy"], m["obstacles"], g))
    return maps, heurs


def _goal_pairs(map_goal):
    seen, out = set(), []
    for m, g in map_goal:
        if g is not None and (id(m), tuple(g)) not in seen:
            seen.add((id(m), tuple(g)))
            out.append((m, tuple(g)))
    return out


def _outcome(r):
    return (r.status, r.cost if r.success else None, r.fmin if r.success else None, r.expanded, r.states, r.actions,
            r.action_costs, r.tier)


def _search_ta(eng, cases, ids):
    from libmultirobotplanning_amd import ll
    maps, heurs = ids
    jobs = [ll.LLJob(map_id=maps[id(m)], algo=ll.ASTAR_TA, start=s, goal=g, vertex_constraints=vc, edge_constraints=ec,
                     max_expansions=cap, heuristic_id=-1 if g is None else heurs[(id(m), tuple(g))])
            for m, s, g, vc, ec, cap, _ in cases]
    return eng.search_batch(jobs)


def _compare_ta(cases, res):
    from libmultirobotplanning_amd import ll
    for (m, s, g, vc, ec, cap, o), r in zip(cases, res):
        assert r.status not in (ll.CAP_NODES, ll.CAP_HORIZON, ll.BAD_JOB), (s, g, r.status)
        if o["rc"] == -1:
            assert r.status == ll.CAP_EXPANSIONS
            continue
        assert (r.success, r.expanded) == (o["success"], o["expanded"]), (s, g, r.expanded, o["expanded"])
        if o["success"]:
            assert r.status == ll.OK
            assert (r.cost, r.fmin, r.states, r.actions, r.action_costs) == (
                o["cost"], o["fmin"], o["states"], o["actions"], o["action_costs"]), (s, g)
        else:
            assert r.status == ll.NO_SOLUTION


def test_astar_ta_searches_uploaded_and_computed_ids_agree(oracle_mod, ref_tests, bench_instances):
    """MRP_LL_ASTAR_TA, both tiers: the same jobs with uploaded and with computed heuristic ids give the same status, cost,
    fmin, expansion count, path and action costs — and the oracle's (oracle/ta_restated.hpp)."""
    from libmultirobotplanning_amd import ll
    cases = _ta_cases(oracle_mod, ref_tests, bench_instances)
    assert len(cases) >= 130
    pairs = _goal_pairs((c[0], c[2]) for c in cases)
    got = []
    for computed in (False, True):
        eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=256)
        try:
            res = _search_ta(eng, cases, _heuristic_ids(eng, pairs, computed, [c[0] for c in cases]))
        finally:
            eng.close()
        _compare_ta(cases, res)
        got.append([_outcome(r) for r in res])
    assert got[0] == got[1]
    assert {o[-1] for o in got[1]} == {0, 1}  # the LDS tier and the arena tier both ran


@pytest.fixture(scope="module")
def eps_ta_cases(ref_tests, bench_instances):
    """MRP_LL_ASTAR_EPS_TA cases as tests/test_ecbs_ta_parity_gpu.py builds them: every low-level call of ecbs_ta.hpp's tree
    over the reference's fixtures and the synthetic corpus (tests/ecbs_ta_corpus.py), each with the CPU checker's answer."""
    cases = []
    for w in (1.0, 1.3):
        for name, inst in ref_tests["cbs_ta"]["inputs"].items():
            m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
            for tasks in _assignments(inst["potential_goals"]):
                _, calls = checker.fixed_tree(m, inst["starts"], tasks, w)
                for c in calls:
                    s = inst["starts"][c["agent"]]
                    o = checker.ll_search(m, s, c["goal"], c["vertex_constraints"], c["edge_constraints"], w=w,
                                          agent_idx=c["agent"], ctx_paths=c["ctx_paths"])
                    cases.append(dict(map=m, start=s, goal=c["goal"], vc=c["vertex_constraints"], ec=c["edge_constraints"],
                                      w=w, agent=c["agent"], ctx=c["ctx_paths"], cap=-1, oracle=o))
    corpus, _ = ecbs_ta_corpus.generate(checker, bench_instances)
    assert len(cases) >= 24 and len(corpus) >= 300
    return cases + corpus


def test_astar_eps_ta_searches_uploaded_and_computed_ids_agree(eps_ta_cases):
    """MRP_LL_ASTAR_EPS_TA (arena tier): uploaded and computed ids give identical results, equal to the checker's."""
    from libmultirobotplanning_amd import ll
    cases = eps_ta_cases
    pairs = _goal_pairs((c["map"], c["goal"]) for c in cases)
    got = []
    for computed in (False, True):
        eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=256)
        try:
            maps, heurs = _heuristic_ids(eng, pairs, computed, [c["map"] for c in cases])
            jobs = [ll.LLJob(map_id=maps[id(c["map"])], algo=ll.ASTAR_EPS_TA, start=c["start"], goal=c["goal"],
                             agent_idx=c["agent"], w=c["w"], vertex_constraints=c["vc"], edge_constraints=c["ec"],
                             ctx_paths=c["ctx"], max_expansions=c["cap"],
                             heuristic_id=-1 if c["goal"] is None else heurs[(id(c["map"]), tuple(c["goal"]))]) for c in cases]
            res = eng.search_batch(jobs)
        finally:
            eng.close()
        for i, (c, r) in enumerate(zip(cases, res)):
            o = c["oracle"]
            assert r.status not in (ll.CAP_NODES, ll.CAP_HORIZON, ll.CAP_FOCAL, ll.BAD_JOB) and r.tier == 1, (i, r.status)
            if o["rc"] == -1:
                assert r.status == ll.CAP_EXPANSIONS, i
                continue
            assert (r.success, r.expanded) == (o["success"], o["expanded"]), (i, r.expanded, o["expanded"])
            if o["success"]:
                assert (r.status, r.cost, r.fmin, r.states, r.actions, r.action_costs) == (
                    ll.OK, o["cost"], o["fmin"], o["states"], o["actions"], o["action_costs"]), i
            else:
                assert r.status == ll.NO_SOLUTION, i
        got.append([_outcome(r) for r in res])
    assert got[0] == got[1]


def test_computed_tables_survive_uploads_and_buffer_growth(oracle_mod, ref_tests, bench_instances):
    """Computed tables live on the device only.  The buffer starts at 2^20 words (4 MB); two batches of twenty 255 x 255
    tables (32 513 words each, 1.3 M words in all) force it to be reallocated while maps, uploaded tables and computed
    tables — those of the first batch too — are in it: every earlier id still reads back unchanged and gives the same
    searches.  After mrp_ll_release_maps the ids start again at 0."""
    from libmultirobotplanning_amd import ll
    cases = _ta_cases(oracle_mod, ref_tests, bench_instances)[:60]
    pairs = _goal_pairs((c[0], c[2]) for c in cases)
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64, max_cells=65025)
    try:
        ids = _heuristic_ids(eng, pairs, True, [c[0] for c in cases])
        first = {h: eng.read_heuristic(h) for h in ids[1].values()}
        for (mk, g), h in ids[1].items():
            m = [p[0] for p in pairs if id(p[0]) == mk][0]
            assert np.array_equal(first[h], hi.bfs(m["dimx"], m["dimy"], m["obstacles"], g))
        before = [_outcome(r) for r in _search_ta(eng, cases, ids)]
        big = hi.random_map(255, 255, 104)
        fc = hi.free_cells(big)
        big_goals = [tuple(fc[0]), tuple(fc[-1]), tuple(fc[len(fc) // 2]), tuple(fc[len(fc) // 3])]
        want_big = {g: hi.bfs(255, 255, big["obstacles"], g) for g in big_goals}
        total_words, big_ids = 0, []
        for batch in range(2):
            extra = hi.random_map(40 + batch, 31, 300 + batch)
            emid = eng.upload_map(extra["dimx"], extra["dimy"], extra["obstacles"])
            eg = tuple(hi.free_cells(extra)[0])
            up = hi.bfs(extra["dimx"], extra["dimy"], extra["obstacles"], eg)
            uh = eng.upload_heuristic(emid, up)
            bmid = eng.upload_map(255, 255, big["obstacles"])
            goals = [big_goals[k % 4] for k in range(20)]
            hids = eng.compute_heuristics([bmid] * 20, [list(g) for g in goals])
            total_words += 20 * ((255 * 255 + 1) // 2)
            big_ids += list(zip(goals, hids))
            assert np.array_equal(eng.read_heuristic(uh), up)
        assert total_words > 2 ** 20  # more than the buffer's first allocation: it has been reallocated
        for g, h in big_ids[:2] + big_ids[18:22] + big_ids[-2:]:
            assert np.array_equal(eng.read_heuristic(h), want_big[g]), (g, h)
        for h, t in first.items():
            assert np.array_equal(eng.read_heuristic(h), t), h
        assert [_outcome(r) for r in _search_ta(eng, cases, ids)] == before
        _compare_ta(cases, _search_ta(eng, cases, ids))
        eng.release_maps()
        m = cases[0][0]
        assert eng.upload_map(m["dimx"], m["dimy"], m["obstacles"]) == 0
        assert eng.compute_heuristics([0, 0], [[0, 0], [3, 0]]) == [0, 1]
        assert np.array_equal(eng.read_heuristic(1), hi.bfs(m["dimx"], m["dimy"], m["obstacles"], (3, 0)))
    finally:
        eng.close()


def test_lookup_is_the_assignment_cost_matrix(bench_instances):
    """heuristic_lookup of every (start, goal) pair equals the tables' entries; INT32_MAX where unreachable."""
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        inst = bench_instances["map_32by32_obst204_agents50_ex3"]
        pocket, pocket_goals = [x for x in hi.small_inputs() if x[0]["dimx"] == 20][0]
        m48 = hi.random_map(48, 48, 101)
        fc48 = hi.free_cells(m48)
        for m, starts, goals, computed in ((inst, inst["starts"], inst["goals"], True),
                                          (pocket, [[0, 0], [11, 11], [12, 13], [19, 16], [9, 9]], pocket_goals, True),
                                          (m48, fc48[::97], fc48[5::301], True),
                                          (inst, inst["starts"][:7], inst["goals"][:5], False)):
            mid = eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
            tabs = [hi.bfs(m["dimx"], m["dimy"], m["obstacles"], g) for g in goals]
            hids = eng.compute_heuristics([mid] * len(goals), goals) if computed else [eng.upload_heuristic(mid, t) for t in tabs]
            q_h = [h for _ in starts for h in hids]
            q_c = [list(s) for s in starts for _ in hids]
            got = eng.heuristic_lookup(q_h, q_c).reshape(len(starts), len(goals))
            want = np.array([[t[s[1], s[0]] for t in tabs] for s in starts], dtype=np.int64)
            assert np.array_equal(got, want)
            if m is pocket:
                assert (got == hi.INF).sum() >= 8 and got[1, 1] == 0
        assert len(eng.heuristic_lookup([], [])) == 0
    finally:
        eng.close()


def test_errors_leave_the_context_unchanged_and_launch_count_is_independent_of_n(bench_instances):
    """MRP_LL_E_INVALID (NULL pointer, unknown map / heuristic id, goal or cell outside its map) and MRP_LL_E_BUSY (inside
    mrp_ll_session_begin) create no id and leave a working context; n == 0 succeeds; one call is the same number of
    launches (mrp_ll_stats.launches) for 1 and for 4096 tables or entries."""
    from libmultirobotplanning_amd import ll
    inst = bench_instances["map_32by32_obst204_agents10_ex0"]
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    lib, h = eng._lib, eng._h

    def arr(a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
        return a, a.ctypes.data_as(I32P)

    def compute(mids, goals, null=None):
        (m, mp), (g, gp) = arr(mids), arr(goals)
        out = np.full(max(len(m), 1), -7, dtype=np.int32)
        args = [mp, gp, out.ctypes.data_as(I32P)]
        if null is not None:
            args[null] = None
        return lib.mrp_ll_compute_heuristics(h, len(m), *args), out[:len(m)].tolist()

    def lookup(hids, cells, null=None):
        (i, ip), (c, cp) = arr(hids), arr(cells)
        out = np.full(max(len(i), 1), -7, dtype=np.int32)
        args = [ip, cp, out.ctypes.data_as(I32P)]
        if null is not None:
            args[null] = None
        return lib.mrp_ll_heuristic_lookup(h, len(i), *args), out[:len(i)].tolist()

    try:
        mid = eng.upload_map(32, 32, inst["obstacles"])
        g0, g1 = inst["goals"][0], inst["goals"][1]
        want0 = hi.bfs(32, 32, inst["obstacles"], g0)
        h0 = eng.compute_heuristics([mid], [g0])[0]
        assert h0 == 0
        dist = np.zeros(1024, dtype=np.int32)
        bad = [compute([mid], [g1], null=0), compute([mid], [g1], null=1), compute([mid], [g1], null=2),
               compute([mid, 5], [g1, g1]), compute([mid, -1], [g1, g1]), compute([mid, mid], [g1, [32, 0]]),
               compute([mid, mid], [g1, [0, -1]]), compute([mid, mid], [g1, [3, 32]])]
        for rc, out in bad:
            assert rc == E_INVALID and all(v == -7 for v in out), (rc, out)
        assert lib.mrp_ll_read_heuristic(h, 1, dist.ctypes.data_as(I32P)) == E_INVALID  # no id was created
        assert lib.mrp_ll_read_heuristic(h, -1, dist.ctypes.data_as(I32P)) == E_INVALID
        assert lib.mrp_ll_read_heuristic(h, 0, None) == E_INVALID
        assert lookup([0], [[0, 0]], null=0)[0] == E_INVALID and lookup([0], [[0, 0]], null=1)[0] == E_INVALID
        assert lookup([0], [[0, 0]], null=2)[0] == E_INVALID
        assert lookup([0, 1], [[0, 0], [0, 0]])[0] == E_INVALID and lookup([0, -1], [[0, 0], [0, 0]])[0] == E_INVALID
        assert lookup([0, 0], [[0, 0], [32, 0]])[0] == E_INVALID and lookup([0, 0], [[0, 0], [0, -1]])[0] == E_INVALID
        assert lib.mrp_ll_compute_heuristics(None, 0, None, None, None) == E_INVALID
        assert compute([], [])[0] == 0 and lookup([], [])[0] == 0 and compute([mid], [g1], null=0)[0] == E_INVALID
        assert lib.mrp_ll_compute_heuristics(h, -1, None, None, None) == E_INVALID
        # the context still works, and the next id is 1
        assert np.array_equal(eng.read_heuristic(0), want0)
        assert eng.compute_heuristics([mid], [g1]) == [1]
        assert np.array_equal(eng.read_heuristic(1), hi.bfs(32, 32, inst["obstacles"], g1))
        job = ll.LLJob(map_id=mid, algo=ll.ASTAR_TA, start=inst["starts"][0], goal=g0, heuristic_id=0)
        r0 = eng.search_batch([job])[0]
        assert r0.status == ll.OK and r0.cost == want0[inst["starts"][0][1], inst["starts"][0][0]]
        # busy inside a session: nothing is created, and the session still serves searches
        eng.session_begin(16)
        try:
            rc, out = compute([mid], [inst["goals"][2]])
            assert rc == E_BUSY and out == [-7]
            assert lib.mrp_ll_read_heuristic(h, 0, dist.ctypes.data_as(I32P)) == E_BUSY
            assert lookup([0], [[0, 0]])[0] == E_BUSY
            assert _outcome(eng.search_batch([job])[0]) == _outcome(r0)
        finally:
            eng.session_end()
        assert eng.compute_heuristics([mid], [inst["goals"][2]]) == [2]
        assert np.array_equal(eng.read_heuristic(2), hi.bfs(32, 32, inst["obstacles"], inst["goals"][2]))
        assert np.array_equal(eng.read_heuristic(0), want0)
        # launches: one call, the same count for n = 1 and n = 4096
        free = hi.free_cells(dict(dimx=32, dimy=32, obstacles=inst["obstacles"]))
        many = [free[k % len(free)] for k in range(4096)]
        counts = []
        for goals in ([many[0]], many):
            a = eng.stats()["launches"]
            hids = eng.compute_heuristics([mid] * len(goals), goals)
            b = eng.stats()["launches"]
            got = eng.heuristic_lookup(hids, [inst["starts"][0]] * len(hids))
            c = eng.stats()["launches"]
            counts.append((b - a, c - b))
            tabs = {}
            for g, v in zip(goals, got.tolist()):
                if tuple(g) not in tabs:
                    tabs[tuple(g)] = hi.bfs(32, 32, inst["obstacles"], g) if len(tabs) < 40 else None
                if tabs[tuple(g)] is not None:
                    assert v == tabs[tuple(g)][inst["starts"][0][1], inst["starts"][0][0]]
            assert np.array_equal(eng.read_heuristic(hids[-1]), hi.bfs(32, 32, inst["obstacles"], goals[-1]))
        assert counts[0] == counts[1] and counts[0][0] >= 1 and counts[0][1] >= 1, counts
    finally:
        eng.close()


def test_cli_prints_the_reference_examples_value(tmp_path, capsys, ref_tests, bench_instances):
    """`shortest_path_heuristic -i in.yaml` prints getValue((0, 0), (3, 0)) (example/shortest_path_heuristic.cpp:152-153)."""
    from libmultirobotplanning_amd import cli
    inst = ref_tests["cbs_ta"]["inputs"]["mapfta_simple1_a1"]
    big = bench_instances["map_32by32_obst204_agents10_ex0"]
    walled = dict(dimx=6, dimy=3, obstacles=[[2, 0], [2, 1], [2, 2]])
    for k, m in enumerate((inst, big, walled)):
        path = tmp_path / ("in%d.yaml" % k)
        with open(path, "w") as f:
            f.write("map:\n  dimensions: [%d, %d]\n  obstacles:\n" % (m["dimx"], m["dimy"]))
            for o in m["obstacles"]:
                f.write("    - [%d, %d]\n" % (o[0], o[1]))
            f.write("agents:\n  - name: agent0\n    start: [0, 0]\n    potentialGoals:\n      - [3, 0]\n")
        assert cli.main(["shortest_path_heuristic", "-i", str(path)]) == 0
        printed = capsys.readouterr().out.strip().splitlines()
        assert printed == [str(int(hi.bfs(m["dimx"], m["dimy"], m["obstacles"], (3, 0))[0, 0]))], (k, printed)
    assert int(hi.bfs(5, 2, inst["obstacles"], (3, 0))[0, 0]) == 3
