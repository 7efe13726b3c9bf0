"""MRP_LL_ASTAR_EPS_TA on the MI355X: the low level of ECBS with task assignment (AStarEpsilon, a_star_epsilon.hpp:86-285,
over the Environment of example/ecbs_ta.cpp:283-445 — what ecbs_ta.hpp:498-499 instantiates) through the C-ABI against the
CPU checker (tests/support/ecbs_ta_check.cpp), bit for bit: status, cost, fmin, expansion count, states, actions, action
costs.  It is the one search of the reference in which a rediscovered node is re-keyed while it sits in the focal list
(a_star_epsilon.hpp:254-269); the corpus holds such searches on purpose (tests/ecbs_ta_corpus.py)."""
import ctypes

import pytest

import ecbs_ta_checker as checker
import ecbs_ta_corpus

pytestmark = pytest.mark.gpu

E_INVALID = -1


def _jobs(eng, cases, ids):
    from libmultirobotplanning_amd import ll
    maps, heurs = ids
    jobs = []
    for c in cases:
        m, g = c["map"], c["goal"]
        key = id(m)
        if key not in maps:
            maps[key] = eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        hid = -1
        if g is not None:
            hk = (key, tuple(g))
            if hk not in heurs:
                heurs[hk] = eng.upload_heuristic(maps[key], ecbs_ta_corpus.bfs_table(m["dimx"], m["dimy"], m["obstacles"], g))
            hid = heurs[hk]
        jobs.append(ll.LLJob(map_id=maps[key], algo=ll.ASTAR_EPS_TA, start=c["start"], goal=g, agent_idx=c["agent"], w=c["w"],
                             vertex_constraints=c["vc"], edge_constraints=c["ec"], ctx_paths=c["ctx"],
                             max_expansions=c["cap"], heuristic_id=hid))
    return jobs


def _run(eng, cases, ids):
    """One batch through mrp_ll_search_batch (or, inside a session, through the job ring).  Every case is compared; a
    capacity status anywhere fails.  Returns the number of cases."""
    from libmultirobotplanning_amd import ll
    res = eng.search_batch(_jobs(eng, cases, ids))
    assert len(res) == len(cases)
    n = 0
    for i, (c, r) in enumerate(zip(cases, res)):
        o = c["oracle"]
        tag = (i, c["start"], c["goal"], c["w"], len(c["vc"]), len(c["ec"]), r.status)
        assert r.status not in (ll.CAP_NODES, ll.CAP_HORIZON, ll.CAP_FOCAL, ll.BAD_JOB), tag
        assert r.tier == 1, tag
        n += 1
        if o["rc"] == -1:
            assert r.status == ll.CAP_EXPANSIONS, tag
            continue
        assert (r.success, r.expanded) == (o["success"], o["expanded"]), (tag, r.expanded, o["expanded"])
        if o["success"]:
            assert r.status == ll.OK, tag
            assert (r.cost, r.fmin, r.states, r.actions, r.action_costs) == (
                o["cost"], o["fmin"], o["states"], o["actions"], o["action_costs"]), tag
        else:
            assert r.status == ll.NO_SOLUTION, tag
    return n


@pytest.fixture(scope="module")
def corpus(bench_instances):
    cases, generated = ecbs_ta_corpus.generate(checker, bench_instances)
    assert generated >= 3000 and len(cases) >= 300
    return cases


def test_every_low_level_call_of_the_reference_fixtures(ref_tests):
    """Every low-level call of ecbs_ta.hpp's conflict tree over test/mapfta_simple1_a{1,2,3}.yaml, for every assignment, at
    w = 1.0 and w = 1.3; the recorded call replayed through the checker's single search first (same answer)."""
    from libmultirobotplanning_amd import ll
    from test_oracle_known_answers import _ta_assignments
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        cases = []
        for w in (1.0, 1.3):
            for name, inst in ref_tests["cbs_ta"]["inputs"].items():
                m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
                for tasks in _ta_assignments(inst["potential_goals"]):
                    _, calls = checker.fixed_tree(m, inst["starts"], tasks, w)
                    for c in calls:
                        s = inst["starts"][c["agent"]]
                        o = checker.ll_search(m, s, c["goal"], c["vertex_constraints"], c["edge_constraints"], w=w,
                                              agent_idx=c["agent"], ctx_paths=c["ctx_paths"])
                        assert (o["success"], o["cost"], o["fmin"], o["expanded"], o["states"], o["action_costs"]) == (
                            c["success"], c["cost"], c["fmin"], c["expanded"], c["states"], c["action_costs"])
                        cases.append(dict(map=m, start=s, goal=c["goal"], vc=c["vertex_constraints"], ec=c["edge_constraints"],
                                          w=w, agent=c["agent"], ctx=c["ctx_paths"], cap=-1, oracle=o))
        assert _run(eng, cases, ({}, {})) == len(cases) >= 24
    finally:
        eng.close()


def test_synthetic_corpus_batch_and_mixed_session(corpus):
    """The whole corpus as one batch, then its first 100 cases inside a mixed session (maps and heuristic tables are uploaded
    before the session).  The corpus holds at least 12 searches with a decrease-key event, at least 8 of them at w = 1.3 and
    at least 2 at w = 2.0 (where nearly the whole open list is in the focal list, so the re-keyed nodes sit in it), more than
    64 vertex and more than 64 edge constraints, a focal context of more than 128 agents, a 48 x 48 map and expansion caps."""
    from libmultirobotplanning_amd import ll
    dk = [c for c in corpus if c["oracle"]["decrease_keys"] > 0]
    assert len(dk) >= 12
    assert sum(1 for c in dk if c["w"] == 1.3) >= 8
    assert sum(1 for c in dk if c["w"] == 2.0) >= 2
    assert any(len(c["vc"]) > 64 and len(c["ec"]) > 64 for c in corpus)
    assert any(len(c["ctx"]) > 128 for c in corpus) and any(c["map"]["dimx"] == 48 for c in corpus)
    assert any(c["oracle"]["rc"] == -1 for c in corpus) and any(c["goal"] is None for c in corpus)
    assert {c["w"] for c in corpus} == {1.0, 1.3, 2.0}
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=256)
    try:
        ids = ({}, {})
        assert _run(eng, corpus, ids) == len(corpus)
        eng.session_begin(64)
        try:
            assert _run(eng, corpus[:100], ids) == 100
        finally:
            eng.session_end()
    finally:
        eng.close()


def test_jobs_the_algorithm_does_not_take_are_rejected(bench_instances):
    """initial_cost != 0 and path_ids are MRP_LL_BAD_JOB (nothing silently runs as another algorithm); the one-algorithm
    sessions and the occupancy query answer MRP_LL_E_INVALID."""
    from libmultirobotplanning_amd import ll
    inst = bench_instances["map_8by8_obst12_agents8_ex0"]
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        mid = eng.upload_map(inst["dimx"], inst["dimy"], inst["obstacles"])
        g = inst["goals"][0]
        hid = eng.upload_heuristic(mid, ecbs_ta_corpus.bfs_table(inst["dimx"], inst["dimy"], inst["obstacles"], g))
        base = dict(map_id=mid, algo=ll.ASTAR_EPS_TA, start=inst["starts"][0], goal=g, w=1.3, heuristic_id=hid)
        res = eng.search_batch([ll.LLJob(**base), ll.LLJob(initial_cost=1, **base),
                                ll.LLJob(ctx_paths=[[], [[1, 1], [1, 2]]], path_ids=[-1, 0], **base),
                                ll.LLJob(heavy=True, **base)])
        assert res[0].status == ll.OK and res[0].tier == 1
        assert [r.status for r in res[1:]] == [ll.BAD_JOB] * 3
        occ = ctypes.c_int32(0)
        assert eng._lib.mrp_ll_session_begin_algo(eng._h, ll.ASTAR_EPS_TA, 8) == E_INVALID
        assert eng._lib.mrp_ll_session_begin_tiers(eng._h, ll.ASTAR_EPS_TA, 8, 2) == E_INVALID
        assert eng._lib.mrp_ll_session_occupancy(eng._h, ll.ASTAR_EPS_TA, ctypes.byref(occ)) == E_INVALID
    finally:
        eng.close()
