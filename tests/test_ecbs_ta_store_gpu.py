"""MRP_LL_ASTAR_EPS_TA with the device-resident path store on the MI355X: a search leaves its path in a store slot
(result_path_id), later searches name their focal context by slot (path_ids) and the workgroup builds the time-major table
itself (ll_ta.h runJobTaEps, ll_jobs.h buildIdTableInArena); mrp_ll_ta_eps_root_batch_stored leaves a root's paths there.

The yardsticks: the CPU checker (tests/support/ecbs_ta_check.cpp) for the recorded calls of ecbs_ta.hpp's conflict tree and
for single searches, and the same job with its context shipped, which tests/test_ecbs_ta_parity_gpu.py holds against the
checker.  Every comparison is exact: status, cost, fmin, expansion count, states, actions, action costs."""
import random

import pytest

import ecbs_ta_checker as checker

pytestmark = pytest.mark.gpu

OPEN32 = dict(dimx=32, dimy=32, obstacles=[])


def _fields(r):
    return (r.status, r.success, r.cost, r.fmin, r.expanded, r.n_states, r.tier, r.states, r.actions, r.action_costs)


def _xy(r):
    return [s[1:] for s in r.states]


class _Bench:
    """One engine with a path store; maps and heuristic tables by content."""

    def __init__(self, slots=64, store=256, **kw):
        from libmultirobotplanning_amd import ll
        self.ll = ll
        self.eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=slots, **kw)
        self.eng.path_store_reserve(store)
        self.store = store
        self.maps, self.heurs = {}, {}

    def close(self):
        self.eng.close()

    def map_id(self, m):
        key = (m["dimx"], m["dimy"], tuple(map(tuple, m["obstacles"])))
        if key not in self.maps:
            self.maps[key] = self.eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        return self.maps[key]

    def prepare(self, pairs):
        """Heuristic tables of (map, goal) pairs, computed before any session begins."""
        want = []
        for m, g in pairs:
            if g is not None and (self.map_id(m), tuple(g)) not in self.heurs and (self.map_id(m), tuple(g)) not in want:
                want.append((self.map_id(m), tuple(g)))
        if want:
            ids = self.eng.compute_heuristics([k[0] for k in want], [list(k[1]) for k in want])
            self.heurs.update(zip(want, ids))

    def job(self, m, start, goal, agent=0, w=1.3, vc=(), ec=(), ctx=(), ids=None, out=-1, cap=-1, **kw):
        hid = -1 if goal is None else self.heurs[(self.map_id(m), tuple(goal))]
        return self.ll.LLJob(map_id=self.map_id(m), algo=self.ll.ASTAR_EPS_TA, start=start, goal=goal, agent_idx=agent, w=w,
                             vertex_constraints=vc, edge_constraints=ec, ctx_paths=ctx, path_ids=ids, result_path_id=out,
                             max_expansions=cap, heuristic_id=hid, **kw)


def _same_as_checker(r, o, tag):
    from libmultirobotplanning_amd import ll
    assert (r.success, r.expanded) == (o["success"], o["expanded"]), (tag, r.status, r.expanded, o["expanded"])
    if o["success"]:
        assert r.status == ll.OK, tag
        assert (r.cost, r.fmin, r.states, r.actions, r.action_costs) == (o["cost"], o["fmin"], o["states"], o["actions"],
                                                                         o["action_costs"]), tag
    else:
        assert r.status == ll.NO_SOLUTION, tag


# ---- replay ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded(ref_tests):
    """Every low-level call of checker.fixed_tree over test/mapfta_simple1_a{1,2,3}.yaml, every assignment, w = 1.0 and 1.3,
    in call order (a context path is always the result of an earlier call of its tree)."""
    from test_oracle_known_answers import _ta_assignments
    calls = []
    for w in (1.0, 1.3):
        for name, inst in sorted(ref_tests["cbs_ta"]["inputs"].items()):
            m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
            for tasks in _ta_assignments(inst["potential_goals"]):
                _, cs = checker.fixed_tree(m, inst["starts"], tasks, w)
                for c in cs:
                    calls.append(dict(c, map=m, start=inst["starts"][c["agent"]], w=w))
    assert len(calls) >= 24
    return calls


def _replay(b, calls, first_slot):
    """The calls one after the other, contexts by slot, every result stored; returns the results."""
    slot_of, nxt, out = {}, first_slot, []
    for i, c in enumerate(calls):
        ids = []
        for a, p in enumerate(c["ctx_paths"]):
            if a == c["agent"] or not p:
                ids.append(-1)
            else:
                assert tuple(map(tuple, p)) in slot_of, "every context path was produced by an earlier search of this run"
                ids.append(slot_of[tuple(map(tuple, p))])
        sid = nxt % b.store
        nxt += 1
        for k in [k for k, v in slot_of.items() if v == sid]:  # (a slot taken again: its earlier path is gone)
            del slot_of[k]
        r = b.eng.search_batch([b.job(c["map"], c["start"], c["goal"], agent=c["agent"], w=c["w"], vc=c["vertex_constraints"],
                                      ec=c["edge_constraints"], ctx=c["ctx_paths"], ids=ids, out=sid)])[0]
        _same_as_checker(r, dict(c, actions=c["actions"]), ("by id", i, c["agent"], c["w"]))
        assert r.tier == 1
        if r.success:
            slot_of[tuple(tuple(s[1:]) for s in c["states"])] = sid
        out.append(r)
    return out


def test_replay_of_the_reference_trees_by_slot_in_batches_and_in_a_mixed_session(recorded):
    """Contexts by slot, results stored, call by call — once as batches and once inside a mixed session — against the
    recorded calls and against the same jobs with shipped contexts; the session's by-id jobs stage fewer bytes than its
    shipped ones (mrp_ll_get_stats.staged_bytes counts what a session stages)."""
    b = _Bench(slots=16, store=2048)
    try:
        assert len(recorded) <= b.store
        b.prepare([(c["map"], c["goal"]) for c in recorded])
        shipped_jobs = [b.job(c["map"], c["start"], c["goal"], agent=c["agent"], w=c["w"], vc=c["vertex_constraints"],
                              ec=c["edge_constraints"], ctx=c["ctx_paths"]) for c in recorded]
        shipped = b.eng.search_batch(shipped_jobs)
        by_id = _replay(b, recorded, 0)
        assert [_fields(r) for r in by_id] == [_fields(r) for r in shipped]
        assert any(j for c in recorded for j in c["ctx_paths"] if j) and any(c["vertex_constraints"] for c in recorded)
        b.eng.session_begin(16)
        try:
            st0 = b.eng.stats()["staged_bytes"]
            in_session = _replay(b, recorded, 700)  # (other slots than the batches': nothing is read that this run did not write)
            st1 = b.eng.stats()["staged_bytes"]
            shipped2 = b.eng.search_batch(shipped_jobs)
            st2 = b.eng.stats()["staged_bytes"]
        finally:
            b.eng.session_end()
        assert [_fields(r) for r in in_session] == [_fields(r) for r in shipped]
        assert [_fields(r) for r in shipped2] == [_fields(r) for r in shipped]
        print("staged bytes per search over %d searches: by id %.1f, shipped %.1f" % (
            len(recorded), (st1 - st0) / len(recorded), (st2 - st1) / len(recorded)))
        assert 0 < st1 - st0 < st2 - st1
    finally:
        b.close()


# ---- the table build's edges -------------------------------------------------------------------------------------------
def _straight(rng, lo, hi, length):
    """Start and goal `length - 1` steps apart inside [lo, hi]^2 (an open map: the path has `length` states)."""
    while True:
        sx, sy = rng.randrange(lo, hi), rng.randrange(lo, hi)
        dx = rng.randrange(0, length)
        dy = length - 1 - dx
        gx, gy = sx + rng.choice((-1, 1)) * dx, sy + rng.choice((-1, 1)) * dy
        if lo <= gx < hi and lo <= gy < hi:
            return [sx, sy], [gx, gy]


@pytest.fixture(scope="module")
def edges():
    """70 unconstrained searches on an open 32 x 32 map whose paths (at most 9 states, one of exactly 9) stay in slots
    0 .. 69, a path of 13 states in slot 70, a path of one state (start == goal) in slot 71, and five paths on an open
    48 x 48 map in slots 80 .. 84."""
    b = _Bench(slots=64, store=128)
    try:
        rng = random.Random(4)
        pairs = [_straight(rng, 8, 22, 9)] + [_straight(rng, 8, 22, rng.randrange(2, 10)) for _ in range(69)]
        pairs.append(_straight(rng, 8, 22, 13))
        pairs.append(([15, 14], [15, 14]))
        open48 = dict(dimx=48, dimy=48, obstacles=[])
        big = [_straight(rng, 30, 47, 12) for _ in range(5)]
        b.prepare([(OPEN32, g) for _, g in pairs] + [(open48, g) for _, g in big] +
                  [(OPEN32, g) for g in ([26, 14], [6, 15], [15, 20])] + [(open48, [46, 40])])
        res = b.eng.search_batch([b.job(OPEN32, s, g, out=k) for k, (s, g) in enumerate(pairs)] +
                                 [b.job(open48, s, g, out=80 + k) for k, (s, g) in enumerate(big)])
        assert all(r.success for r in res)
        paths = [_xy(r) for r in res]
        assert [len(p) for p in paths[70:72]] == [13, 1] and max(len(p) for p in paths[:70]) == 9 == len(paths[0])
        yield b, paths[:72], paths[72:], open48
    finally:
        b.close()


def _by_id_and_shipped(b, m, start, goal, agent, ctx, ids, **kw):
    return [b.job(m, start, goal, agent=agent, ctx=ctx, ids=ids, **kw), b.job(m, start, goal, agent=agent, ctx=ctx, **kw)]


def test_table_build_edges(edges):
    """Two chunks of the agent loop with a searching agent in the middle (71 agents: rows of 80 cells), t_pad 9 and 13 (no
    multiples of 8), a 1-state path, an empty path, a lone agent (no table), an agent without a task, a 48 x 48 map, more than
    64 vertex and edge constraints: each by id against the checker (given the stored paths) and against its shipped twin."""
    b, paths, paths48, open48 = edges
    rng = random.Random(9)
    cases = []

    def add(name, m, start, goal, agent, ctx, ids, w=1.3, vc=(), ec=()):
        cases.append((name, m, start, goal, agent, ctx, vc, ec, w, _by_id_and_shipped(b, m, start, goal, agent, ctx, ids, w=w, vc=vc, ec=ec)))

    def around(agent, pool):  # the searching agent at index `agent`, the pool's paths around it
        ctx = [paths[k] for k in pool[:agent]] + [[]] + [paths[k] for k in pool[agent:]]
        ids = list(pool[:agent]) + [-1] + list(pool[agent:])
        return ctx, ids

    ctx, ids = around(35, list(range(70)))
    add("70 agents, t_pad 9", OPEN32, [6, 14], [26, 14], 35, ctx, ids)
    add("70 agents, t_pad 9, w 1", OPEN32, [6, 14], [26, 14], 35, ctx, ids, w=1.0)
    ctx, ids = around(35, list(range(1, 70)) + [70])
    add("70 agents, t_pad 13", OPEN32, [24, 15], [6, 15], 35, ctx, ids)
    ctx, ids = around(2, [71, 0, 5])
    ctx[1], ids[1] = [], -1  # an empty path beside the 1-state path
    add("1-state and empty paths", OPEN32, [15, 8], [15, 20], 2, ctx, ids)
    add("lone agent", OPEN32, [15, 8], [15, 20], 0, [[]], [-1])
    ctx, ids = around(3, list(range(20)))
    add("no goal", OPEN32, paths[7][0], None, 3, ctx, ids, vc=[[3, paths[7][0][0], paths[7][0][1]]])
    free = [(x, y) for x in range(8, 24) for y in range(8, 24)]
    vc = [[rng.randrange(1, 12)] + list(rng.choice(free)) for _ in range(70)]
    ec = []
    while len(ec) < 70:
        x, y = rng.choice(free)
        dx, dy = rng.choice(((1, 0), (-1, 0), (0, 1), (0, -1)))
        ec.append([rng.randrange(0, 12), x, y, x + dx, y + dy])
    ctx, ids = around(9, list(range(30, 70)))
    add("70 + 70 constraints", OPEN32, [6, 14], [26, 14], 9, ctx, ids, vc=vc, ec=ec)
    ctx48 = paths48[:2] + [[]] + paths48[2:]
    add("48 x 48", open48, [30, 40], [46, 40], 2, ctx48, [80, 81, -1, 82, 83, 84])
    assert len(cases[0][5]) == 71 and len(cases[0][5]) % 16 != 0
    res = b.eng.search_batch([j for c in cases for j in c[9]])
    for k, (name, m, start, goal, agent, ctx, vc, ec, w, _) in enumerate(cases):
        o = checker.ll_search(m, start, goal, vc, ec, w=w, agent_idx=agent, ctx_paths=ctx)
        _same_as_checker(res[2 * k], o, name)
        assert _fields(res[2 * k]) == _fields(res[2 * k + 1]), name
    # the contexts are seen: at w = 1.3 the search through 70 agents differs from the search with nobody there
    alone = checker.ll_search(OPEN32, [6, 14], [26, 14], w=1.3)
    assert (alone["expanded"], alone["states"]) != (res[0].expanded, res[0].states)


# ---- a recycled slot ---------------------------------------------------------------------------------------------------
def test_a_rewritten_slot_is_read_as_rewritten():
    """Slot 3 holds a long path and is read; then another search leaves a shorter path there and a reader in a LATER batch,
    and a later job of the same session, see the short one (the store is read with agent-scope loads: a stale cache line
    would show as the long path's expansion count or route)."""
    b = _Bench(slots=8, store=8)
    try:
        long_sg, short_sg, reader = ([4, 14], [22, 14]), ([14, 10], [14, 13]), ([22, 14], [4, 14])
        b.prepare([(OPEN32, g) for _, g in (long_sg, short_sg, reader)])

        def write(sg):
            r = b.eng.search_batch([b.job(OPEN32, sg[0], sg[1], out=3)])[0]
            assert r.success
            return _xy(r)

        def read(ctx_path, tag):
            got, twin = b.eng.search_batch(_by_id_and_shipped(b, OPEN32, reader[0], reader[1], 1, [ctx_path, []], [3, -1]))
            o = checker.ll_search(OPEN32, reader[0], reader[1], w=1.3, agent_idx=1, ctx_paths=[ctx_path, []])
            _same_as_checker(got, o, tag)
            assert _fields(got) == _fields(twin), tag
            return got

        def round_trip(tag):
            long_path = write(long_sg)
            r_long = read(long_path, tag + ": long")
            short_path = write(short_sg)
            r_short = read(short_path, tag + ": short")
            assert len(long_path) == 19 and len(short_path) == 4
            assert (r_long.expanded, r_long.states) != (r_short.expanded, r_short.states), "the two contents tell apart"

        round_trip("batches")
        b.eng.session_begin(8)
        try:
            round_trip("one session")
        finally:
            b.eng.session_end()
    finally:
        b.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refused_jobs_leave_their_neighbours_alone(edges):
    b, paths, _, _ = edges
    ll = b.ll
    ctx, ids = [paths[0], [], paths[1]], [0, -1, 1]
    good = _by_id_and_shipped(b, OPEN32, [6, 14], [26, 14], 1, ctx, ids)[0]
    want = _fields(b.eng.search_batch([good])[0])
    bad = [b.job(OPEN32, [6, 14], [26, 14], agent=1, ctx=ctx, ids=[b.store, -1, 1]),      # id >= slots
           b.job(OPEN32, [6, 14], [26, 14], agent=1, ctx=ctx, ids=ids, out=b.store),      # result slot out of range
           b.job(OPEN32, [6, 14], [26, 14], agent=1, ctx=ctx, ids=ids, heavy=True),
           b.job(OPEN32, [6, 14], [26, 14], agent=1, ctx=ctx, ids=ids),                   # (MRP_LL_JOB_ROOT_CHAIN, set below)
           b.job(OPEN32, [6, 14], [26, 14], agent=1, ctx=ctx, ids=ids, initial_cost=1)]
    jobs = [good]
    for j in bad:
        jobs += [j, good]
    cap = b.eng.max_horizon
    cjobs, cres, (keep, states, actions, costs) = b.eng._marshal(jobs, cap)
    cjobs[1 + 2 * 3].flags |= ll.JOB_ROOT_CHAIN
    b.eng._check(b.eng._lib.mrp_ll_search_batch(b.eng._h, len(jobs), cjobs, cres), "mrp_ll_search_batch")
    res = b.eng._results(len(jobs), cap, cres, states, actions, costs)
    assert [r.status for r in res[1::2]] == [ll.BAD_JOB] * 5
    assert all(_fields(r) == want for r in res[0::2])
    # ... and the slots the context names still hold what they held
    assert _fields(b.eng.search_batch([good])[0]) == want


# ---- roots -------------------------------------------------------------------------------------------------------------
def _root_fields(t):
    return (t.planned, [_fields(r) for r in t.results], t.conflict)


def _children(b, world_maps, root, got, ids, agents=None):
    """For the agents of a root (all, or `agents`): a child job with one vertex constraint, the others' paths by slot, and
    its shipped twin; returns (jobs, tags)."""
    n = len(root.starts)
    jobs, tags = [], []
    for a in (agents if agents is not None else range(n)):
        ctx = [_xy(r) if (q != a and r.success) else [] for q, r in enumerate(got.results)]
        pid = [ids[q] if ctx[q] else -1 for q in range(n)]
        own = _xy(got.results[a]) if got.results[a].success else [root.starts[a]]
        vc = [[1, own[min(1, len(own) - 1)][0], own[min(1, len(own) - 1)][1]]]
        for form in (pid, None):
            jobs.append(b.ll.LLJob(map_id=root.map_id, algo=b.ll.ASTAR_EPS_TA, start=root.starts[a], goal=root.goals[a], agent_idx=a,
                                   w=1.3, vertex_constraints=vc, ctx_paths=ctx, path_ids=form, heuristic_id=root.heuristic_ids[a]))
        tags.append((n, a))
    return jobs, tags


def test_roots_leave_their_paths_in_the_store():
    """Roots of 1, 3, 16, 17 and 40 agents: the call with slot ids returns what the call without returns, and child jobs
    over the stored roots equal their shipped twins.  A root that ends behind an agent leaves the slots of the agents it did
    not plan as they were."""
    from test_ta_eps_root_gpu import _World, _random_map
    b = _Bench(slots=4, store=128)
    try:
        eng, ll = b.eng, b.ll
        world = _World(eng)
        m16, comp = _random_map(16, 16, 30, 5)
        for n in (1, 3, 16, 17, 40):
            rng = random.Random(300 + n)
            world.add("n%d" % n, "m16", m16, rng.sample(comp, n), rng.sample(comp, n))
        pocket = dict(dimx=6, dimy=6, obstacles=[[3, 4], [5, 4], [4, 3], [4, 5]])
        world.add("unreachable_mid", "pocket", pocket, [(0, 0), (1, 0), (2, 0)], [(2, 2), (4, 4), (5, 0)])
        world.add("filler", "pocket", pocket, [(0, 5), (1, 5)], [(0, 1), (1, 1)])
        roots = world.finish()
        filler = eng.ta_eps_root_batch(roots[6:], 1.3, result_path_ids=[[101, 102]])[0]  # what slots 101 and 102 hold beforehand
        assert filler.planned == 2 and all(r.success for r in filler.results)
        plain = eng.ta_eps_root_batch(roots[:6], 1.3)
        ids, nxt = [], 0
        for r in roots[:5]:
            ids.append(list(range(nxt, nxt + len(r.starts))))
            nxt += len(r.starts)
        ids[1][1] = -1  # an agent whose path is not stored
        ids.append([100, 101, 102])
        stored = eng.ta_eps_root_batch(roots[:6], 1.3, result_path_ids=ids)
        assert [_root_fields(t) for t in stored] == [_root_fields(t) for t in plain]
        assert [t.planned for t in stored[:5]] == [1, 3, 16, 17, 40] and stored[5].planned == 2
        assert stored[5].results[0].success and not stored[5].results[1].success and stored[5].results[2].status == ll.NOT_RUN
        jobs, tags = [], []
        for r, t, i in zip(roots[:5], stored[:5], ids[:5]):
            pick = None if len(r.starts) <= 3 else [0, len(r.starts) // 2, len(r.starts) - 1]
            if i is ids[1]:
                pick = [1]  # (the agent whose own path is not stored: every OTHER path is)
            j, g = _children(b, world.maps, r, t, i, pick)
            jobs += j
            tags += g
        res = eng.search_batch(jobs)
        for k, tag in enumerate(tags):
            assert res[2 * k].status in (ll.OK, ll.NO_SOLUTION) and _fields(res[2 * k]) == _fields(res[2 * k + 1]), tag
        # the root that ended behind agent 1: slot 100 holds agent 0's path, slots 101 and 102 still the filler's
        bad = roots[5]
        ctx = [_xy(stored[5].results[0]), _xy(filler.results[0]), _xy(filler.results[1]), []]
        pair = [ll.LLJob(map_id=bad.map_id, algo=ll.ASTAR_EPS_TA, start=[5, 0], goal=[2, 2], agent_idx=3, w=1.3, ctx_paths=ctx,
                         path_ids=form, heuristic_id=bad.heuristic_ids[0]) for form in ([100, 101, 102, -1], None)]
        got, twin = eng.search_batch(pair)
        assert got.success and _fields(got) == _fields(twin)
        # a slot outside the store refuses the root, and only that root
        out = eng.ta_eps_root_batch(roots[:2], 1.3, result_path_ids=[[0], [5, 128, 6]])
        assert _root_fields(out[0]) == _root_fields(plain[0])
        assert out[1].planned == 0 and all(r.status == ll.BAD_JOB for r in out[1].results)
    finally:
        b.close()


def test_a_root_the_host_finishes_stores_its_paths_too(monkeypatch):
    """Under MRP_LL_ARENA_PATHS_BYTES=4096 a 17-agent root whose last paths have 63, 65 and 67 states outgrows the path area:
    the kernel stops behind agent 15 and the call plans agent 16 as an ordinary job.  Every slot is readable afterwards."""
    from test_ta_eps_root_gpu import _World, _snake
    monkeypatch.setenv("MRP_LL_ARENA_PATHS_BYTES", "4096")
    b = _Bench(slots=2, store=32)
    try:
        eng, ll = b.eng, b.ll
        world = _World(eng)
        snake, order = _snake(16, 6)
        long3 = [(order[0], order[62]), (order[10], order[74]), (order[20], order[86])]
        short = [(order[30 + 3 * a], order[32 + 3 * a]) for a in range(14)]
        world.add("long_last", "snake", snake, [p[0] for p in short + long3], [p[1] for p in short + long3])
        root, = world.finish()
        plain, = eng.ta_eps_root_batch([root], 1.3)
        ids = list(range(5, 22))
        stored, = eng.ta_eps_root_batch([root], 1.3, result_path_ids=[ids])
        assert _root_fields(stored) == _root_fields(plain) and stored.planned == 17
        assert [r.n_states for r in stored.results[14:]] == [63, 65, 67]
        # one reader per slot (a table of 17 agents and 67 rows does not fit this path area; one of 2 agents does)
        jobs = []
        for a in range(17):
            for form in ([ids[a], -1], None):
                jobs.append(ll.LLJob(map_id=root.map_id, algo=ll.ASTAR_EPS_TA, start=list(order[30]), goal=list(order[62]), agent_idx=1,
                                     w=1.3, ctx_paths=[_xy(stored.results[a]), []], path_ids=form, heuristic_id=root.heuristic_ids[14]))
        res = eng.search_batch(jobs)
        for a in range(17):
            assert res[2 * a].success and _fields(res[2 * a]) == _fields(res[2 * a + 1]), a
        # ... and the whole context by id is refused here: 67 rows of 32 cells are more than 4096 bytes
        whole = ll.LLJob(map_id=root.map_id, algo=ll.ASTAR_EPS_TA, start=root.starts[0], goal=root.goals[0], agent_idx=0, w=1.3,
                         ctx_paths=[[]] + [_xy(r) for r in stored.results[1:]], path_ids=[-1] + ids[1:], heuristic_id=root.heuristic_ids[0])
        assert eng.search_batch([whole])[0].status == ll.BAD_JOB
    finally:
        b.close()
