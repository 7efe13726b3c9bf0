"""mrp_ll_submit_scan on the MI355X: a flagged A*-epsilon job also returns the conflicts of the conflict-tree node it completes.

The reference answer everywhere is the oracle's conflict_scan (getFirstConflict ecbs.cpp:401-452 + focalHeuristic :315-350)
of the solution S assembled here, in Python: S[agent] = the path the flagged search returned, S[j] = the path another
search left in path-store slot path_ids[j].  The engine's own conflict_scan kernel has to agree as well, and the job's
result has to be what the same job returns without the flag.  Every status is checked, none is filtered on.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("found", "time", "agent1", "agent2", "type", "x1", "y1", "x2", "y2", "count")
NO_SCAN = dict(zip(KEYS, (-1,) + (0,) * 9))
W = 1.3
OBST_8 = [[2, 2], [2, 5], [5, 2], [5, 5], [3, 6]]  # single cells apart from each other: they enclose nothing


@pytest.fixture(scope="module")
def engine():
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1)
    eng.path_store_reserve(2048)
    yield eng
    eng.close()


def _instance(dim, n_agents, obstacles, seed):
    """Distinct random starts and distinct random goals on the free cells; agent 1 starts on its goal."""
    rng = np.random.RandomState(seed)
    free = [[x, y] for y in range(dim) for x in range(dim) if [x, y] not in obstacles]
    starts = [free[i] for i in rng.permutation(len(free))[:n_agents]]
    goals = [free[i] for i in rng.permutation(len(free))[:n_agents]]
    if n_agents > 1:
        if starts[1] in goals:
            goals[goals.index(starts[1])] = goals[1]
        goals[1] = starts[1]
    return dict(dimx=dim, dimy=dim, obstacles=obstacles, starts=starts, goals=goals)


def _xy(result):
    return [s[1:] for s in result.states]


class Node:
    """A conflict-tree node in the path store: every agent planned alone (slot = agent), then one child job per agent."""

    def __init__(self, eng, inst, slot0=0, late_goal_agent=None):
        from libmultirobotplanning_amd import ll
        self.ll, self.eng, self.inst, self.n, self.slot0 = ll, eng, inst, len(inst["starts"]), slot0
        self.mid = eng.upload_map(inst["dimx"], inst["dimy"], inst["obstacles"])
        alone = eng.search_batch([ll.LLJob(map_id=self.mid, algo=ll.ASTAR_EPS, start=inst["starts"][a], goal=inst["goals"][a],
                                           agent_idx=a, w=W, result_path_id=slot0 + a) for a in range(self.n)])
        assert [r.status for r in alone] == [ll.OK] * self.n
        self.paths = [_xy(r) for r in alone]
        self.cons = []
        longest = max(len(p) for p in self.paths)
        for a, p in enumerate(self.paths):
            if a == late_goal_agent:  # the goal cell is taken at a late time: the new path outlasts every other
                self.cons.append([[longest + 3] + inst["goals"][a]])
            elif len(p) >= 2:         # one cell of the stored path, at its time
                k = max(1, len(p) // 2)
                self.cons.append([[k] + p[k]])
            else:
                self.cons.append([])

    def jobs(self, scan=True, heavy=False, out_base=None, agents=None, **over):
        ll = self.ll
        out_base = self.slot0 + self.n if out_base is None else out_base
        out = []
        for a in (range(self.n) if agents is None else agents):
            ids = [self.slot0 + b if b != a else -1 for b in range(self.n)]
            kw = dict(map_id=self.mid, algo=ll.ASTAR_EPS, start=self.inst["starts"][a], goal=self.inst["goals"][a], agent_idx=a,
                      w=W, vertex_constraints=self.cons[a], ctx_paths=self.paths, path_ids=ids, result_path_id=out_base + a,
                      scan_conflicts=scan, heavy=heavy)
            kw.update(over)
            out.append(ll.LLJob(**kw))
        return out

    def expected(self, oracle_mod, agent, result):
        S = list(self.paths)
        S[agent] = _xy(result)
        return S, oracle_mod.conflict_scan(S)


def _same_result(a, b):
    return (a.status, a.cost, a.fmin, a.n_states, a.expanded, a.states, a.actions, a.tier) == \
        (b.status, b.cost, b.fmin, b.n_states, b.expanded, b.states, b.actions, b.tier)


def _check_node(eng, oracle_mod, node, **job_args):
    """One flagged job per agent of `node`; returns (results, conflicts) after comparing with the oracle, the engine's own
    scan kernel and the unflagged jobs."""
    ll = node.ll
    res, conf = eng.search_batch_scan(node.jobs(**job_args))
    plain = eng.search_batch(node.jobs(scan=False, **{k: v for k, v in job_args.items() if k != "scan"}))
    sols = []
    for a in range(node.n):
        assert res[a].status == ll.OK, (a, res[a].status)
        S, want = node.expected(oracle_mod, a, res[a])
        assert conf[a] == want, (a, conf[a], want)
        assert _same_result(res[a], plain[a]), a
        sols.append(S)
    assert eng.conflict_scan(sols) == conf
    return res, conf


@pytest.mark.parametrize("dim,n_agents,obstacles,seed", [(8, 4, OBST_8, 1), (8, 12, OBST_8, 2), (32, 70, [], 3), (32, 130, [], 4)])
def test_batch_mode(engine, oracle_mod, dim, n_agents, obstacles, seed):
    """Agents 0, 63, 64 and the last one are among the searching agents of the wide nodes (two and three lane chunks); agent 1
    starts on its goal (a single-state path in everybody's context); agent 2's new path is the longest of its node."""
    inst = _instance(dim, n_agents, obstacles, seed)
    node = Node(engine, inst, late_goal_agent=2)
    assert len(node.paths[1]) == 1
    res, conf = _check_node(engine, oracle_mod, node)
    assert res[2].n_states > max(len(p) for p in node.paths)
    assert n_agents < 70 or any(c["found"] == 1 for c in conf)  # (paths planned alone: dozens of agents do collide)
    # 130 agents: a table row of 144 columns is beyond the LDS tier's 128, every search is the arena tier's; the smaller
    # nodes' searches start in the LDS tier, whose table is in LDS for 4 and 12 agents and in the arena slot for 70
    assert {r.tier for r in res} == {1} if n_agents > 128 else 0 in {r.tier for r in res}


def test_single_agent_and_swap(engine, oracle_mod):
    from libmultirobotplanning_amd import ll
    # a node of one agent has no pair: found = 0, count = 0
    one = dict(dimx=8, dimy=8, obstacles=OBST_8, starts=[[0, 0]], goals=[[7, 7]])
    mid = engine.upload_map(8, 8, OBST_8)
    res, conf = engine.search_batch_scan([ll.LLJob(map_id=mid, algo=ll.ASTAR_EPS, start=one["starts"][0], goal=one["goals"][0],
                                                   agent_idx=0, w=W, ctx_paths=[[]], path_ids=[-1], scan_conflicts=True)])
    assert res[0].status == ll.OK
    assert conf[0] == dict(zip(KEYS, (0,) * 10))
    # two agents that change places: the first conflict of every child of this node is the edge between them
    swap = dict(dimx=8, dimy=8, obstacles=[], starts=[[1, 0], [2, 0], [6, 6]], goals=[[2, 0], [1, 0], [6, 7]])
    node = Node(engine, swap, slot0=100)
    node.cons = [[], [], [[1, 6, 7]]]
    res, conf = _check_node(engine, oracle_mod, node)
    for a in range(3):
        assert (conf[a]["found"], conf[a]["type"], conf[a]["time"], conf[a]["agent1"], conf[a]["agent2"]) == (1, 1, 0, 0, 1)
        assert (conf[a]["x1"], conf[a]["y1"], conf[a]["x2"], conf[a]["y2"]) == (1, 0, 2, 0)


def test_tiers_and_sessions(oracle_mod):
    """The same flagged jobs in the mixed session, the A*-epsilon session and the front / heavy session, finishing in the LDS
    tier (0), the arena tier (1: MRP_LL_JOB_HEAVY under an all-tier kernel) and a heavy workgroup's wide tier (2): the
    conflicts are the oracle's in all of them; an engine without an LDS tier gives them from the arena as well."""
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    tiers = set()
    try:
        eng.path_store_reserve(1024)
        small = Node(eng, _instance(8, 12, OBST_8, 2), slot0=0, late_goal_agent=2)
        wide = Node(eng, _instance(32, 70, [], 3), slot0=100, late_goal_agent=2)
        base = {}
        for node in (small, wide):
            res, conf = _check_node(eng, oracle_mod, node)
            base[node] = conf
            tiers |= {r.tier for r in res}
        for begin in (lambda: eng.session_begin(32), lambda: eng.session_begin_algo(ll.ASTAR_EPS, 32),
                      lambda: eng.session_begin_tiers(32, 4)):
            begin()
            try:
                for node in (small, wide):
                    for heavy in (False, True):
                        res, conf = _check_node(eng, oracle_mod, node, heavy=heavy)
                        assert conf == base[node]
                        tiers |= {r.tier for r in res}
            finally:
                eng.session_end()
        assert eng.stats()["heavy_fallbacks"] == 0
    finally:
        eng.close()
    assert tiers == {0, 1, 2}
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64, lds_nodes=-1)
    try:
        eng.path_store_reserve(256)
        node = Node(eng, _instance(8, 12, OBST_8, 2), late_goal_agent=2)
        res, conf = _check_node(eng, oracle_mod, node)
        assert conf == base[small] and {r.tier for r in res} == {1}
    finally:
        eng.close()


def test_no_scan_without_a_path(engine, oracle_mod):
    from libmultirobotplanning_amd import ll
    node = Node(engine, _instance(8, 4, OBST_8, 1), slot0=200)
    x, y = node.inst["starts"][0]
    walled = [[1, x + dx, y + dy] for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))]
    jobs = node.jobs(agents=[0], vertex_constraints=walled) + node.jobs(agents=[3], max_expansions=1) + \
        node.jobs(agents=[3], scan=False) + node.jobs(agents=[3])
    res, conf = engine.search_batch_scan(jobs)
    assert [r.status for r in res] == [ll.NO_SOLUTION, ll.CAP_EXPANSIONS, ll.OK, ll.OK]
    assert conf[0] == NO_SCAN and conf[1] == NO_SCAN
    assert conf[2] == dict(zip(KEYS, (ll.SCAN_UNTOUCHED,) * 10))
    assert conf[3] == node.expected(oracle_mod, 3, res[3])[1]


def _submit_scan_with_flags(eng, jobs, more_flags):
    """search_batch_scan with further MRP_LL_JOB_* bits or-ed into the marshalled jobs' flags."""
    import ctypes
    from libmultirobotplanning_amd import ll
    n, cap = len(jobs), eng.max_horizon
    cjobs, cres, (keep, states, actions, costs) = eng._marshal(jobs, cap)
    for i, f in enumerate(more_flags):
        cjobs[i].flags |= f
    conf = (ll.mrp_ll_conflict * n)()
    ticket = ctypes.c_int32(-1)
    assert eng._lib.mrp_ll_submit_scan(eng._h, 0, n, cjobs, cres, conf, ctypes.byref(ticket)) == 0
    assert eng._lib.mrp_ll_wait(eng._h, ticket.value) == 0
    return (eng._results(n, cap, cres, states, actions, costs),
            [{k: getattr(conf[i], k) for k, _ in ll.mrp_ll_conflict._fields_} for i in range(n)])


def test_rejections(oracle_mod):
    """Every condition of a valid flagged job (include/mrp_ll.h), one at a time: MRP_LL_BAD_JOB, no conflicts, and the valid
    job beside it runs and is scanned as usual."""
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        inst = _instance(8, 4, OBST_8, 1)
        # no path store reserved: the context is not accepted by id
        mid = eng.upload_map(8, 8, OBST_8)
        res, conf = eng.search_batch_scan([ll.LLJob(map_id=mid, algo=ll.ASTAR_EPS, start=[0, 0], goal=[7, 7], agent_idx=0, w=W,
                                                    ctx_paths=[[]], path_ids=[-1], scan_conflicts=True)])
        assert res[0].status == ll.BAD_JOB and conf[0] == NO_SCAN
        eng.path_store_reserve(256)
        node = Node(eng, inst)
        good = node.jobs(agents=[3])[0]
        others_empty = [[]] + node.paths[1:]
        bad = [
            node.jobs(agents=[0], algo=ll.ASTAR)[0],
            node.jobs(agents=[0], path_ids=None)[0],
            node.jobs(agents=[0], ctx_paths=[], path_ids=[])[0],                       # n_agents == 0
            node.jobs(agents=[0], agent_idx=-1)[0],
            node.jobs(agents=[0], agent_idx=4)[0],
            node.jobs(agents=[0], path_ids=[-1, 1, -1, 3])[0],                         # another agent without a slot
            node.jobs(agents=[1], ctx_paths=others_empty, path_ids=[0, -1, 2, 3])[0],  # another agent with an empty path
            node.jobs(agents=[0], path_ids=[-1, 1, 2, 99999])[0],                      # a slot the store does not have
        ]
        for k, job in enumerate(bad):
            res, conf = eng.search_batch_scan([job, good])
            assert res[0].status == ll.BAD_JOB, k
            assert conf[0] == NO_SCAN, k
            assert res[1].status == ll.OK and conf[1] == node.expected(oracle_mod, 3, res[1])[1], k
        # a flagged job that is also a root chain: LLJob has no such combination, so the flag goes into the marshalled job
        res, conf = _submit_scan_with_flags(eng, [node.jobs(agents=[0])[0], good], [ll.JOB_ROOT_CHAIN, 0])
        assert res[0].status == ll.BAD_JOB and conf[0] == NO_SCAN
        assert res[1].status == ll.OK and conf[1] == node.expected(oracle_mod, 3, res[1])[1]
        # a flagged job is admitted by mrp_ll_submit_scan alone: any other entry point rejects it, in a batch and in a session
        res = eng.search_batch([good, node.jobs(agents=[3], scan=False)[0]])
        assert [r.status for r in res] == [ll.BAD_JOB, ll.OK]
        eng.session_begin_algo(ll.ASTAR_EPS, 16)
        try:
            res = eng.search_batch([good, node.jobs(agents=[3], scan=False)[0]])
            assert [r.status for r in res] == [ll.BAD_JOB, ll.OK]
            res, conf = eng.search_batch_scan([bad[0], good])
            assert res[0].status == ll.BAD_JOB and conf[0] == NO_SCAN
            assert res[1].status == ll.OK and conf[1] == node.expected(oracle_mod, 3, res[1])[1]
        finally:
            eng.session_end()
    finally:
        eng.close()


def test_lds_windows_are_what_they_were_before_the_scan():
    """The scan passes its job and its answer through spare bytes of the window's control block and is a function of its own
    behind the search: the resident kernels ask for the LDS they asked for before it existed — 10 880 bytes of narrow
    window (ll_compact.h, A*-epsilon kernels) plus the default 4 096 of path table, 31 360 for a heavy workgroup — and the
    runtime grants them the residency it granted then: ten front workgroups per CU beside the heavy ones, eight per CU for
    an A*-epsilon session, seven for a mixed or A* one."""
    import ctypes
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0)
    try:
        occ, front, heavy = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        assert eng._lib.mrp_ll_session_tiers_geometry(eng._h, ctypes.byref(occ), ctypes.byref(front), ctypes.byref(heavy)) == 0
        assert (front.value, heavy.value) == (10880 + 4096, 31360)
        # the answers of the commit before the scan on an MI355X (DESIGN.md section 3 "Conflict scans")
        assert occ.value == 10
        assert (eng.session_occupancy(ll.ASTAR_EPS), eng.session_occupancy(ll.ASTAR)) == (8, 7)
    finally:
        eng.close()


def _digest(paths):
    import hashlib
    h = hashlib.sha256()
    for p in paths:
        h.update(("|" + ",".join("%d:%d" % (x, y) for x, y in p)).encode())
    return h.hexdigest()[:16]


def test_driver_with_device_scans(monkeypatch, bench_instances, oracle_expected):
    """The ECBS session driver with MRP_HL_DEVICE_SCAN=1 — children flagged, their conflicts taken from the answers — against
    the same driver with the variable unset: both give the oracle's cost, makespan, expansion counts and schedule."""
    from libmultirobotplanning_amd import hl
    names = ["map_32by32_obst204_agents10_ex%d" % k for k in range(20)] + \
        ["map_32by32_obst204_agents%d_ex%d" % (a, k) for a in (20, 30) for k in range(10)] + ["map_32by32_obst204_agents50_ex0"]
    scans = {}
    s = hl.BatchSolver(device=0, n_threads=2, slots=512)
    try:
        for on in (False, True):
            if on:
                monkeypatch.setenv("MRP_HL_DEVICE_SCAN", "1")
            else:
                monkeypatch.delenv("MRP_HL_DEVICE_SCAN", raising=False)
            res, st = s.solve([bench_instances[n] for n in names], algo=hl.ECBS, w=1.3)
            for n, r in zip(names, res):
                e = oracle_expected[n]["ecbs_w1.3"]
                assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"], _digest(r["paths"])) == (
                    hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"], e["digest"]), (n, on)
            scans[on] = st["device_scans"]
    finally:
        s.close()
    assert scans[False] == 0 and scans[True] > 0
