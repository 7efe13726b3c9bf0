"""mrp_ll_submit_node on the MI355X: a job flagged MRP_LL_JOB_SCAN_FROM_PARENT returns the conflicts of the conflict-tree child
it completes, worked out from what the parent node's scan established.

The expected answer everywhere is the oracle's conflict_scan of the CHILD, assembled here in Python as test_node_scan_gpu.py
does: S[agent] = the path the flagged search returned, S[j] = the path in path-store slot path_ids[j].  The engine's own
conflict_scan kernel and the same job with MRP_LL_JOB_SCAN_CONFLICTS alone have to agree, and the job's result has to be the
unflagged job's.  The bases come from the oracle's scan of the PARENT node (every agent's stored path).  Every status is
checked, none is filtered on.  Seeds are fixed; they were chosen through the oracle (search results are bit-exact with it) so
that the case set holds every branch of the scan, which test_case_set_reaches_every_branch asserts.
"""
import numpy as np
import pytest

from test_node_scan_gpu import KEYS, NO_SCAN, OBST_8, W, Node, _digest, _instance, _same_result, _xy

pytestmark = pytest.mark.gpu

# name -> (dim, agents, obstacles, seed, late_goal_agent, long_parent_agent, the agents that search, {agent: its constraints})
CASES = {
    "8x8_2": (8, 2, OBST_8, 25, None, None, None, {}),
    "8x8_3": (8, 3, OBST_8, 13, None, None, None, {}),
    "8x8_6": (8, 6, OBST_8, 5, None, None, None, {}),
    "8x8_6_new_path_longest": (8, 6, OBST_8, 5, 2, None, None, {}),      # T_new > T_old: the full-scan fallback
    "8x8_6_old_path_longest": (8, 6, OBST_8, 5, None, 3, None, {}),      # T_new < T_old: the other direction
    # a constraint that sends the new path into another agent BEFORE the parent's first conflict (t = 4 and t = 3): with
    # agent 0 the pair is (a, j), an edge; with agent 2 a vertex; with agent 5 the pair is (j, a), an edge: j's move
    "8x8_6_early_own": (8, 6, OBST_8, 18, None, None, None, {0: [[2, 2, 4]], 2: [[1, 2, 4]]}),
    "8x8_6_early_own_low": (8, 6, OBST_8, 19, None, None, None, {5: [[1, 1, 3]]}),
    "32x32_65": (32, 65, [], 3, None, None, (0, 63, 64), {}),            # two lane chunks, the table in memory
    "32x32_130": (32, 130, [], 4, None, None, (0, 63, 64, 129), {}),     # three
}
MODES = ("zero", "first")  # clean_before = 0, = the parent's first-conflict time


class ParentNode(Node):
    """test_node_scan_gpu.Node as the PARENT of the children its jobs complete: slot0 + a holds agent a's path at the parent.
    long_parent_agent: that agent's parent path is one that reaches its goal late, so the child's (planned without the late
    constraint) is shorter and the node's horizon shrinks."""

    def __init__(self, eng, inst, slot0=0, late_goal_agent=None, long_parent_agent=None):
        super().__init__(eng, inst, slot0=slot0, late_goal_agent=late_goal_agent)
        if long_parent_agent is not None:
            a, ll = long_parent_agent, self.ll
            late = [[max(len(p) for p in self.paths) + 3] + inst["goals"][a]]
            r = eng.search_batch([ll.LLJob(map_id=self.mid, algo=ll.ASTAR_EPS, start=inst["starts"][a], goal=inst["goals"][a],
                                           agent_idx=a, w=W, vertex_constraints=late, result_path_id=slot0 + a)])[0]
            assert r.status == ll.OK
            self.paths[a] = _xy(r)
            assert len(self.paths[a]) == max(len(p) for p in self.paths)
            self.cons[a] = []

    def parent_scan(self, oracle_mod):
        return oracle_mod.conflict_scan(self.paths)

    def base(self, oracle_mod, mode):
        p = self.parent_scan(oracle_mod)
        horizon = max(len(q) for q in self.paths) - 1
        return (p["count"], 0 if mode == "zero" else (p["time"] if p["found"] == 1 else horizon))

    def node_jobs(self, oracle_mod, mode, agents=None, **over):
        out = []
        for a in (range(self.n) if agents is None else agents):
            ids = [self.slot0 + b for b in range(self.n)]  # the searching agent's entry: the slot of the path it replaces
            out += self.jobs(agents=[a], path_ids=ids, scan_base=self.base(oracle_mod, mode), **over)
        return out


def _make(eng, name, slot0):
    dim, n, obst, seed, late, long_parent, agents, cons = CASES[name]
    node = ParentNode(eng, _instance(dim, n, obst, seed), slot0=slot0, late_goal_agent=late, long_parent_agent=long_parent)
    for a, c in cons.items():
        node.cons[a] = c
    return node, (list(range(n)) if agents is None else list(agents))


def _but_tier(r):
    return (r.status, r.cost, r.fmin, r.n_states, r.expanded, r.states, r.actions)


@pytest.fixture(scope="module")
def engine():
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    eng.path_store_reserve(2048)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def batch(engine, oracle_mod):
    """Every case in batch mode, once: name -> (node, agents, {mode: (results, conflicts)}), each compared with the oracle's
    scan of the child, the engine's scan kernel, the MRP_LL_JOB_SCAN_CONFLICTS-only job and the unflagged job."""
    from libmultirobotplanning_amd import ll
    out, slot0 = {}, 0
    for name in CASES:
        node, agents = _make(engine, name, slot0)
        slot0 += 2 * node.n
        scan_only = engine.search_batch_scan(node.jobs(agents=agents))
        plain = engine.search_batch(node.jobs(scan=False, agents=agents))
        per_mode = {}
        for mode in MODES:
            res, conf = engine.search_batch_scan(node.node_jobs(oracle_mod, mode, agents=agents))
            sols = []
            for k, a in enumerate(agents):
                assert res[k].status == ll.OK, (name, mode, a, res[k].status)
                S, want = node.expected(oracle_mod, a, res[k])
                assert conf[k] == want, (name, mode, a, conf[k], want)
                assert conf[k] == scan_only[1][k], (name, mode, a)
                assert _same_result(res[k], plain[k]) and _same_result(res[k], scan_only[0][k]), (name, mode, a)
                sols.append(S)
            assert engine.conflict_scan(sols) == conf, (name, mode)
            per_mode[mode] = (res, conf)
        out[name] = (node, agents, per_mode)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_batch_mode(batch, name):
    """The fixture has compared every word; here: the shapes are what the case names say."""
    node, agents, per_mode = batch[name]
    dim, n, obst, seed, late, long_parent, _, _ = CASES[name]
    res = per_mode["zero"][0]
    others = lambda a: max(len(p) for b, p in enumerate(node.paths) if b != a)
    if n >= 2 and dim == 8:
        assert len(node.paths[1]) == 1  # the agent that starts on its goal, as a searching agent and in every context
    if late is not None:
        k = agents.index(late)
        assert max(res[k].n_states, others(late)) > max(len(node.paths[late]), others(late))
    if long_parent is not None:
        k = agents.index(long_parent)
        assert max(res[k].n_states, others(long_parent)) < max(len(node.paths[long_parent]), others(long_parent))
    if n > 64:
        assert {r.tier for r in res} == ({1} if n > 128 else {0})  # (130 agents: beyond the LDS tier's 128 columns)


def test_case_set_reaches_every_branch(batch, oracle_mod):
    seen = set()
    for name, (node, agents, per_mode) in batch.items():
        for mode in MODES:
            res, conf = per_mode[mode]
            clean_before = node.base(oracle_mod, mode)[1]
            for k, a in enumerate(agents):
                others = max(len(p) for b, p in enumerate(node.paths) if b != a)
                t_new, t_old = max(others, res[k].n_states), max(others, len(node.paths[a]))
                if t_new > t_old:
                    seen.add("fallback, the new path outlasts")
                elif t_new < t_old:
                    seen.add("fallback, the old path outlasted")
                elif conf[k]["found"] == 0:
                    seen.add("no conflict")
                elif a not in (conf[k]["agent1"], conf[k]["agent2"]):
                    seen.add("first conflict among others")
                elif conf[k]["time"] < clean_before:
                    seen.add("first conflict with the replaced agent before clean_before")
    assert seen == {"fallback, the new path outlasts", "fallback, the old path outlasted", "no conflict",
                    "first conflict among others", "first conflict with the replaced agent before clean_before"}


def _through(engine, oracle_mod, batch, names, **job_args):
    for name in names:
        node, agents, per_mode = batch[name]
        for mode in MODES:
            res, conf = engine.search_batch_scan(node.node_jobs(oracle_mod, mode, agents=agents, **job_args))
            assert [r.status for r in res] == [0] * len(agents), (name, mode)
            assert conf == per_mode[mode][1], (name, mode)
            assert [_but_tier(r) for r in res] == [_but_tier(r) for r in per_mode[mode][0]], (name, mode)


def test_sessions(engine, oracle_mod, batch):
    """The same jobs in a mixed session, an A*-epsilon session and a front / heavy pair with the front tables in LDS and in
    device memory, and once with MRP_LL_JOB_HEAVY: the conflicts and results of the batch."""
    from libmultirobotplanning_amd import ll
    names = list(CASES)
    for begin in (lambda: engine.session_begin(32), lambda: engine.session_begin_algo(ll.ASTAR_EPS, 32)):
        begin()
        try:
            _through(engine, oracle_mod, batch, names)
        finally:
            engine.session_end()
    for in_memory in (False, True):
        engine.session_front_tables(in_memory)
        engine.session_begin_tiers(32, 4)
        try:
            _through(engine, oracle_mod, batch, names)
            if in_memory:
                _through(engine, oracle_mod, batch, ["8x8_6", "32x32_65"], heavy=True)
        finally:
            engine.session_end()
    engine.session_front_tables(False)
    assert engine.stats()["heavy_fallbacks"] == 0


def _submit_node_raw(eng, jobs, bases, more_flags=None, with_bases=True, with_conf=True):
    import ctypes
    from libmultirobotplanning_amd import ll
    n, cap = len(jobs), eng.max_horizon
    cjobs, cres, (keep, states, actions, costs) = eng._marshal(jobs, cap)
    for i, f in enumerate(more_flags or []):
        cjobs[i].flags = f
    conf = (ll.mrp_ll_conflict * n)()
    for c in conf:
        for k in KEYS:
            setattr(c, k, ll.SCAN_UNTOUCHED)
    cb = (ll.mrp_ll_scan_base * n)()
    for i, b in enumerate(bases):
        cb[i].parent_count, cb[i].clean_before = b
    ticket = ctypes.c_int32(-1)
    assert eng._lib.mrp_ll_submit_node(eng._h, 0, n, cjobs, cres, conf if with_conf else None, None, cb if with_bases else None,
                                       ctypes.byref(ticket)) == 0
    assert eng._lib.mrp_ll_wait(eng._h, ticket.value) == 0
    return (eng._results(n, cap, cres, states, actions, costs), [{k: getattr(conf[i], k) for k in KEYS} for i in range(n)])


def test_rejections_and_unflagged_jobs(engine, oracle_mod, batch):
    """Every condition include/mrp_ll.h adds for the flag, one at a time: MRP_LL_BAD_JOB, found = -1, and the valid job beside
    it runs and is scanned; an unflagged job of the call ignores bases[i]; the flag through another entry point is rejected."""
    from libmultirobotplanning_amd import ll
    node, agents, per_mode = batch["8x8_6"]
    base = node.base(oracle_mod, "first")
    good = node.node_jobs(oracle_mod, "first", agents=[3])[0]
    want3 = per_mode["first"][1][agents.index(3)]
    ids = [node.slot0 + b for b in range(node.n)]
    no_own = list(ids); no_own[0] = -1
    far_own = list(ids); far_own[0] = 99999
    empty_own = [[]] + node.paths[1:]
    flags = ll.JOB_SCAN_CONFLICTS | ll.JOB_SCAN_FROM_PARENT | ll.JOB_STORE_RESULT
    bad = [
        (node.jobs(agents=[0], path_ids=no_own, scan_base=base)[0], base, None),        # no slot for the replaced path
        (node.jobs(agents=[0], path_ids=far_own, scan_base=base)[0], base, None),       # a slot the store does not have
        (node.jobs(agents=[0], path_ids=ids, ctx_paths=empty_own, scan_base=base)[0], base, None),  # path_len[agent_idx] == 0
        (node.jobs(agents=[0], path_ids=ids, scan_base=base)[0], (-1, 0), None),        # parent_count < 0
        (node.jobs(agents=[0], path_ids=ids, scan_base=base)[0], (0, -1), None),        # clean_before < 0
        (node.jobs(agents=[0], path_ids=ids, scan_base=base)[0], base, flags & ~ll.JOB_SCAN_CONFLICTS),  # the flag alone
        (node.jobs(agents=[0], path_ids=ids, scan_base=base, algo=ll.ASTAR)[0], base, None),
        (node.jobs(agents=[0], path_ids=[-1 if b == 2 else s for b, s in enumerate(ids)], scan_base=base)[0], base, None),
    ]
    for k, (job, b, f) in enumerate(bad):
        res, conf = _submit_node_raw(engine, [job, good], [b, base], more_flags=None if f is None else [f, flags])
        assert res[0].status == ll.BAD_JOB, k
        assert conf[0] == (NO_SCAN if (f is None or f & ll.JOB_SCAN_CONFLICTS) else dict(zip(KEYS, (ll.SCAN_UNTOUCHED,) * 10))), k
        assert res[1].status == ll.OK and conf[1] == want3, k
    # bases == NULL: flagged jobs are rejected, unflagged ones run; an unflagged job ignores bases[i]
    scan_only = node.jobs(agents=[3])[0]
    res, conf = _submit_node_raw(engine, [good, scan_only], [base, base], with_bases=False)
    assert [r.status for r in res] == [ll.BAD_JOB, ll.OK] and conf[1] == want3
    res, conf = _submit_node_raw(engine, [scan_only], [(-7, -7)])
    assert res[0].status == ll.OK and conf[0] == want3
    # the flag through mrp_ll_submit_scan / mrp_ll_submit: rejected, in a batch and in a session
    import ctypes
    for session in (False, True):
        if session:
            engine.session_begin_algo(ll.ASTAR_EPS, 16)
        try:
            n, cap = 2, engine.max_horizon
            cjobs, cres, bufs = engine._marshal([good, scan_only], cap)
            conf = (ll.mrp_ll_conflict * n)()
            ticket = ctypes.c_int32(-1)
            assert engine._lib.mrp_ll_submit_scan(engine._h, 0, n, cjobs, cres, conf, ctypes.byref(ticket)) == 0
            assert engine._lib.mrp_ll_wait(engine._h, ticket.value) == 0
            assert (cres[0].status, cres[1].status) == (ll.BAD_JOB, ll.OK)
            assert {k: getattr(conf[1], k) for k in KEYS} == want3
            cjobs, cres, bufs = engine._marshal([good, node.jobs(agents=[3], scan=False)[0]], cap)
            assert engine._lib.mrp_ll_submit(engine._h, n, cjobs, cres, ctypes.byref(ticket)) == 0
            assert engine._lib.mrp_ll_wait(engine._h, ticket.value) == 0
            assert (cres[0].status, cres[1].status) == (ll.BAD_JOB, ll.OK)
        finally:
            if session:
                engine.session_end()


def test_single_agent_and_failed_search(engine, oracle_mod, batch):
    """n_agents == 1: found 0, count 0.  A search that ends without a path: found = -1, the rest 0."""
    from libmultirobotplanning_amd import ll
    mid = engine.upload_map(8, 8, OBST_8)
    alone = engine.search_batch([ll.LLJob(map_id=mid, algo=ll.ASTAR_EPS, start=[0, 0], goal=[7, 7], agent_idx=0, w=W,
                                          result_path_id=2000)])[0]
    res, conf = engine.search_batch_scan([ll.LLJob(map_id=mid, algo=ll.ASTAR_EPS, start=[0, 0], goal=[7, 7], agent_idx=0, w=W,
                                                   ctx_paths=[_xy(alone)], path_ids=[2000], scan_conflicts=True, scan_base=(0, 0))])
    assert res[0].status == ll.OK and conf[0] == dict(zip(KEYS, (0,) * 10))
    node, agents, per_mode = batch["8x8_6"]
    x, y = node.inst["starts"][0]
    walled = [[1, x + dx, y + dy] for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))]
    res, conf = engine.search_batch_scan(node.node_jobs(oracle_mod, "first", agents=[0], vertex_constraints=walled) +
                                         node.node_jobs(oracle_mod, "first", agents=[3], max_expansions=1))
    assert [r.status for r in res] == [ll.NO_SOLUTION, ll.CAP_EXPANSIONS]
    assert conf == [NO_SCAN, NO_SCAN]


def test_geometry_and_occupancy_are_the_parents():
    """The new wave program is a function of its own behind the search and adds no LDS: the resident kernels get the windows
    and the residency they had before it (the figures test_node_scan_gpu.py pins, plus the two task-assignment kinds)."""
    import ctypes
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0)
    try:
        occ, front, heavy = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        assert eng._lib.mrp_ll_session_tiers_geometry(eng._h, ctypes.byref(occ), ctypes.byref(front), ctypes.byref(heavy)) == 0
        assert (occ.value, front.value, heavy.value) == (10, 10880 + 4096, 31360)
        assert (eng.session_occupancy(ll.ASTAR_EPS), eng.session_occupancy(ll.ASTAR)) == (8, 7)
    finally:
        eng.close()


def test_driver_with_incremental_scans(monkeypatch, bench_instances, oracle_expected):
    """The ECBS session driver with MRP_HL_DEVICE_SCAN_INCREMENTAL=1, with MRP_HL_DEVICE_SCAN=1 and with neither: the oracle's
    cost, makespan, expansion counts and schedule in all three, incremental_scans > 0 only with the new variable, and the same
    number of low-level expansions."""
    from libmultirobotplanning_amd import hl
    names = ["map_32by32_obst204_agents10_ex%d" % k for k in range(20)] + \
        ["map_32by32_obst204_agents%d_ex%d" % (a, k) for a in (20, 30) for k in range(10)] + ["map_32by32_obst204_agents50_ex0"]
    stats = {}
    s = hl.BatchSolver(device=0, n_threads=2, slots=512)
    try:
        for knob in (None, "MRP_HL_DEVICE_SCAN", "MRP_HL_DEVICE_SCAN_INCREMENTAL"):
            monkeypatch.delenv("MRP_HL_DEVICE_SCAN", raising=False)
            monkeypatch.delenv("MRP_HL_DEVICE_SCAN_INCREMENTAL", raising=False)
            if knob:
                monkeypatch.setenv(knob, "1")
            res, st = s.solve([bench_instances[n] for n in names], algo=hl.ECBS, w=1.3)
            for n, r in zip(names, res):
                e = oracle_expected[n]["ecbs_w1.3"]
                assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"], _digest(r["paths"])) == (
                    hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"], e["digest"]), (n, knob)
            stats[knob] = st
    finally:
        s.close()
    assert stats[None]["device_scans"] == 0 and stats[None]["incremental_scans"] == 0
    assert stats["MRP_HL_DEVICE_SCAN"]["device_scans"] > 0 and stats["MRP_HL_DEVICE_SCAN"]["incremental_scans"] == 0
    inc = stats["MRP_HL_DEVICE_SCAN_INCREMENTAL"]
    assert inc["incremental_scans"] > 0 and inc["device_scans"] >= inc["incremental_scans"]
    assert len({st["ll_expansions"] for st in stats.values()}) == 1
