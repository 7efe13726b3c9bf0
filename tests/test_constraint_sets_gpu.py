"""The device-resident constraint store on the MI355X (mrp_ll_constraint_store_reserve / mrp_ll_submit_sets).

A job that names its agent's set by a store slot and ships only what it adds has to return exactly what the same job
returns with the whole union shipped in its arrays: every case here is compared with the oracle (a_star.hpp /
a_star_epsilon.hpp restated) on the flattened set AND with the flat job sent through mrp_ll_submit, field by field, path
and tier included.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

W = 1.3
MOVES = [(-1, 0), (1, 0), (0, 1), (0, -1)]
OBST_8 = [[2, 2], [2, 5], [5, 2], [5, 5], [3, 6]]
OBST_40 = [[x, 11] for x in range(4, 30)] + [[20, y] for y in range(14, 22)] + [[33, 5], [34, 5], [35, 6]]
MAPS = {
    "8x8": dict(dimx=8, dimy=8, obstacles=OBST_8, start=[0, 0], goal=[7, 6], other=[[7, 0], [6, 0], [5, 0], [4, 0], [4, 1], [4, 2]]),
    # dimensions above 32: the arena tier, and an edge word that holds y * dimx + x with dimx != dimy
    "40x24": dict(dimx=40, dimy=24, obstacles=OBST_40, start=[1, 2], goal=[37, 20],
                  other=[[36, 20], [36, 19], [36, 18], [35, 18], [34, 18], [34, 17]]),
}


def _fields(r):
    return (r.status, r.cost, r.fmin, r.n_states, r.expanded, r.states, r.actions, r.tier)


def _vs_oracle(oracle_mod, ll, algo, mp, agent, start, goal, vc, ec, ctx, w, r, cap=-1, what=None):
    o = oracle_mod.ll_search(oracle_mod.ASTAR_EPS if algo == ll.ASTAR_EPS else oracle_mod.ASTAR, mp, agent, start, goal, vc, ec,
                             ctx, w=w, cap_expansions=cap)
    if o["rc"] == -1:
        assert r.status == ll.CAP_EXPANSIONS, what
        return o
    assert (r.success, r.expanded) == (o["success"], o["expanded"]), what
    if o["success"]:
        assert (r.status, r.cost, r.fmin, r.states, r.actions) == (ll.OK, o["cost"], o["fmin"], o["states"], o["actions"]), what
    else:
        assert r.status == ll.NO_SOLUTION, what
    return o


def _free_cells(mp):
    return [[x, y] for y in range(mp["dimy"]) for x in range(mp["dimx"]) if [x, y] not in mp["obstacles"]]


def _random_vertex(rng, free, tmax=24):
    return [rng.randrange(1, tmax)] + rng.choice(free)


def _random_edge(rng, mp, free, tmax=24):
    while True:
        c = rng.choice(free)
        dx, dy = rng.choice(MOVES)
        if 0 <= c[0] + dx < mp["dimx"] and 0 <= c[1] + dy < mp["dimy"]:
            return [rng.randrange(0, tmax), c[0], c[1], c[0] + dx, c[1] + dy]


@pytest.mark.parametrize("eps", [False, True])
@pytest.mark.parametrize("map_name", ["8x8", "40x24"])
def test_chains_in_a_batch(oracle_mod, map_name, eps):
    """One chain, every step a call of its own that adds one seeded constraint to the previous step's result set: 65 vertex
    constraints (the compact tier loads 64 per pass: 63 / 64 / 65), then 65 edge constraints (beyond 64 a job leaves the
    compact tier: the tier changes exactly where the flat job's does), then one more word, which fills the slot
    (words_per_slot = 131) — and one beyond it, which is MRP_LL_BAD_JOB."""
    from libmultirobotplanning_amd import ll
    mp = MAPS[map_name]
    rng = random.Random(7 + len(map_name) + 2 * eps)
    free = _free_cells(mp)
    algo = ll.ASTAR_EPS if eps else ll.ASTAR
    w = W if eps else 1.0
    ctx = [[], mp["other"]] if eps else []  # a two-agent shipped focal context
    words = 131
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        eng.constraint_store_reserve(3, words)
        mid = eng.upload_map(mp["dimx"], mp["dimy"], mp["obstacles"])
        kw = dict(map_id=mid, algo=algo, start=mp["start"], goal=mp["goal"], agent_idx=0, w=w, ctx_paths=ctx)
        vc, ec, by_set, flat_jobs, sets = [], [], [], [], []
        for depth in range(1, words + 1):
            p = by_set[-1].states if by_set and by_set[-1].status == ll.OK and depth % 3 == 0 else []
            k = rng.randrange(1, len(p) - 1) if len(p) >= 3 else 0  # every third constraint: a step of the path just found
            if depth <= 65 or depth == words:
                add_v, add_e = [[k] + p[k][1:] if k else _random_vertex(rng, free)], []
            else:
                add_v, add_e = [], [[k] + p[k][1:] + p[k + 1][1:] if k else _random_edge(rng, mp, free)]
            vc, ec = vc + add_v, ec + add_e
            r = eng.search_batch([ll.LLJob(vertex_constraints=add_v, edge_constraints=add_e,
                                           base_set_id=(depth - 1) % 3 if depth > 1 else -1, result_set_id=depth % 3, **kw)])[0]
            by_set.append(r)
            sets.append((list(vc), list(ec)))
            flat_jobs.append(ll.LLJob(vertex_constraints=vc, edge_constraints=ec, **kw))
        # the slot is full: one more word does not fit, the job is not run and creates no set
        r = eng.search_batch([ll.LLJob(vertex_constraints=[_random_vertex(rng, free)], base_set_id=words % 3,
                                       result_set_id=(words + 1) % 3, **kw)])[0]
        assert r.status == ll.BAD_JOB
        flat = eng.search_batch(flat_jobs)  # mrp_ll_search_batch: mrp_ll_submit + mrp_ll_wait
        for depth, (r, f, (v, e)) in enumerate(zip(by_set, flat, sets), start=1):
            assert _fields(r) == _fields(f), (depth, _fields(r)[:5], _fields(f)[:5])
            _vs_oracle(oracle_mod, ll, algo, mp, 0, mp["start"], mp["goal"], v, e, ctx, w, r, what=depth)
        tiers = [r.tier for r in by_set]
        if map_name == "8x8":  # 65 vertex + 64 edge constraints still run in the compact tier, the 65th edge constraint ends that
            assert tiers[:3] == [0] * 3 and tiers[128] == 0 and tiers[129:] == [1] * 2, tiers
        else:
            assert tiers == [1] * words
        assert len({str(r.states) for r in by_set}) > 5  # (the constraints do bite)
    finally:
        eng.close()


@pytest.mark.parametrize("eps", [False, True])
def test_last_goal_constraint_lives_in_the_set(oracle_mod, eps):
    """m_lastGoalConstraint (ecbs.cpp:268-273) of the union: the goal-cell constraint sits in the BASE, the job adds a
    constraint elsewhere.  Once at time 5 (the agent may not stay on its goal before time 6), once at a time beyond the
    horizon — dropped as a word (the two-word slot below would otherwise be too small), but it still counts: the search
    cannot end, and runs into its expansion cap exactly as the oracle's does."""
    from libmultirobotplanning_amd import ll
    mp = dict(dimx=8, dimy=8, obstacles=OBST_8)
    start, goal = [0, 0], [3, 0]
    algo = ll.ASTAR_EPS if eps else ll.ASTAR
    w = W if eps else 1.0
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        eng.constraint_store_reserve(4, 2)
        mid = eng.upload_map(8, 8, OBST_8)
        kw = dict(map_id=mid, algo=algo, start=start, goal=goal, agent_idx=0, w=w, max_expansions=2000)
        elsewhere = [[1, 1, 0]]
        for slot, goal_cons in ((0, [[5] + goal]), (2, [[5] + goal, [eng.max_horizon + 88] + goal])):
            base = eng.search_batch([ll.LLJob(vertex_constraints=goal_cons, result_set_id=slot, **kw)])[0]
            _vs_oracle(oracle_mod, ll, algo, mp, 0, start, goal, goal_cons, [], [], w, base, cap=2000, what=("base", slot))
            r = eng.search_batch([ll.LLJob(vertex_constraints=elsewhere, base_set_id=slot, result_set_id=slot + 1, **kw)])[0]
            f = eng.search_batch([ll.LLJob(vertex_constraints=goal_cons + elsewhere, **kw)])[0]
            assert _fields(r) == _fields(f), (slot, _fields(r)[:5], _fields(f)[:5])
            o = _vs_oracle(oracle_mod, ll, algo, mp, 0, start, goal, goal_cons + elsewhere, [], [], w, r, cap=2000, what=slot)
            if slot == 0:
                assert r.status == ll.OK and r.cost == o["cost"] >= 6
            else:
                assert o["rc"] == -1 and r.status == ll.CAP_EXPANSIONS
    finally:
        eng.close()


def _chains_in_a_session(oracle_mod, bench_instances, begin, algos):
    """64 independent chains of depth 24, one job of every chain per call (so the steps of a chain interleave with the other
    chains' and land on whichever of the 256 workgroups is free); result slots come from a pool of 192 handed round first in,
    first out, so every slot is written and read several times, by different chains."""
    from libmultirobotplanning_amd import ll
    inst = bench_instances["map_32by32_obst204_agents10_ex0"]
    mp = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
    free = _free_cells(mp)
    n_chains, depth_max = 64, 24
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=256)
    try:
        eng.constraint_store_reserve(192, 64)
        mid = eng.upload_map(mp["dimx"], mp["dimy"], mp["obstacles"])
        rng = random.Random(99)
        chains = []
        for c in range(n_chains):
            a, b = c % 10, (c + 1 + c // 10) % 10
            algo = algos[c % len(algos)]
            other = oracle_mod.ll_search(oracle_mod.ASTAR, mp, 0, inst["starts"][b], inst["goals"][b])
            chains.append(dict(algo=algo, w=W if algo == ll.ASTAR_EPS else 1.0, start=inst["starts"][a], goal=inst["goals"][a],
                               ctx=[[], [s[1:] for s in other["states"]]] if algo == ll.ASTAR_EPS else [],
                               vc=[], ec=[], slot=-1, last=None))
        pool = list(range(192))
        used = [0] * 192
        begin(eng)
        try:
            done = []  # (chain, vc, ec, result)
            for depth in range(depth_max):
                jobs = []
                for ch in chains:
                    p = ch["last"].states if ch["last"] is not None and ch["last"].status == ll.OK else []
                    add_v, add_e = [], []
                    if len(p) >= 3 and rng.random() < 0.8:  # what a conflict tree adds: a step of the path just found
                        k = rng.randrange(1, len(p) - 1)
                        if rng.random() < 0.5:
                            add_v = [[k] + p[k][1:]]
                        else:
                            add_e = [[k] + p[k][1:] + p[k + 1][1:]]
                    elif rng.random() < 0.5:
                        add_v = [_random_vertex(rng, free)]
                    else:
                        add_e = [_random_edge(rng, mp, free)]
                    ch["vc"], ch["ec"] = ch["vc"] + add_v, ch["ec"] + add_e
                    ch["new"] = pool.pop(0)
                    used[ch["new"]] += 1
                    jobs.append(ll.LLJob(map_id=mid, algo=ch["algo"], start=ch["start"], goal=ch["goal"], agent_idx=0, w=ch["w"],
                                         ctx_paths=ch["ctx"], vertex_constraints=add_v, edge_constraints=add_e,
                                         base_set_id=ch["slot"], result_set_id=ch["new"]))
                res = eng.search_batch(jobs)
                for ch, r in zip(chains, res):
                    if ch["slot"] >= 0:
                        pool.append(ch["slot"])
                    ch["slot"], ch["last"] = ch["new"], r
                    done.append((ch, list(ch["vc"]), list(ch["ec"]), r))
            assert min(used) >= 4  # every slot of the pool has been several chains' result
            flat = []
            for lo in range(0, len(done), 512):
                flat += eng.search_batch([ll.LLJob(map_id=mid, algo=ch["algo"], start=ch["start"], goal=ch["goal"], agent_idx=0,
                                                   w=ch["w"], ctx_paths=ch["ctx"], vertex_constraints=vc, edge_constraints=ec)
                                          for ch, vc, ec, _ in done[lo:lo + 512]])
        finally:
            eng.session_end()
        for i, ((ch, vc, ec, r), f) in enumerate(zip(done, flat)):
            assert _fields(r) == _fields(f), (i, _fields(r)[:5], _fields(f)[:5])
            _vs_oracle(oracle_mod, ll, ch["algo"], mp, 0, ch["start"], ch["goal"], vc, ec, ch["ctx"], ch["w"], r, what=i)
        assert sum(1 for _, _, _, r in done if r.status == ll.OK) > len(done) // 2
    finally:
        eng.close()


def test_sets_cross_workgroups_in_a_mixed_session(oracle_mod, bench_instances):
    from libmultirobotplanning_amd import ll
    _chains_in_a_session(oracle_mod, bench_instances, lambda eng: eng.session_begin(256), [ll.ASTAR, ll.ASTAR_EPS])


def test_sets_cross_workgroups_in_an_eps_session(oracle_mod, bench_instances):
    from libmultirobotplanning_amd import ll
    _chains_in_a_session(oracle_mod, bench_instances, lambda eng: eng.session_begin_algo(ll.ASTAR_EPS, 256), [ll.ASTAR_EPS])


def test_front_and_heavy_pair(oracle_mod):
    """A search with a base set that outgrows the narrow tier: the front workgroup stages the union, writes the result set and
    hands the job over; the heavy workgroup stages again, finds the same base and writes the same words (tier == 2).  A
    follow-up job names that result set."""
    from libmultirobotplanning_amd import ll
    obst = [[x, y] for y in range(1, 12, 2) for x in range(32) if x != (31 if (y // 2) % 2 == 0 else 0)]  # a serpentine
    mp = dict(dimx=32, dimy=32, obstacles=obst)
    start, goal = [0, 0], [0, 12]
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=256)
    try:
        eng.constraint_store_reserve(4, 16)
        mid = eng.upload_map(32, 32, obst)
        kw = dict(map_id=mid, algo=ll.ASTAR_EPS, start=start, goal=goal, agent_idx=0, w=W)
        eng.session_begin_tiers(96, 12)
        try:
            vc, ec, got = [], [], []
            for k in range(3):  # each step constrains the path the step before found
                p = got[-1].states if got else []
                add_v = [[40] + p[40][1:]] if k == 1 else [[3, 3, 0]] if k == 0 else []
                add_e = [[80] + p[80][1:] + p[81][1:]] if k == 2 else []
                vc, ec = vc + add_v, ec + add_e
                r = eng.search_batch([ll.LLJob(vertex_constraints=add_v, edge_constraints=add_e, base_set_id=k - 1,
                                               result_set_id=k, **kw)])[0]
                f = eng.search_batch([ll.LLJob(vertex_constraints=vc, edge_constraints=ec, **kw)])[0]
                assert _fields(r) == _fields(f), (k, _fields(r)[:5], _fields(f)[:5])
                o = _vs_oracle(oracle_mod, ll, ll.ASTAR_EPS, mp, 0, start, goal, vc, ec, [], W, r, what=k)
                assert o["success"] and o["cost"] > 130 and r.tier == 2
                got.append(r)
            assert got[0].states != got[1].states != got[2].states
        finally:
            eng.session_end()
        assert eng.stats()["heavy_active_wgs"] >= 1
    finally:
        eng.close()


def test_with_the_conflict_scan(oracle_mod):
    """MRP_LL_JOB_CONSTRAINT_SET | MRP_LL_JOB_SCAN_CONFLICTS | MRP_LL_JOB_STORE_RESULT on one job: the child of a four-agent
    node whose paths are in the path store."""
    from libmultirobotplanning_amd import ll
    inst = dict(dimx=8, dimy=8, obstacles=OBST_8, starts=[[0, 0], [7, 0], [0, 7], [3, 3]], goals=[[7, 7], [0, 0], [7, 1], [4, 3]])
    n = 4
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        eng.path_store_reserve(16)
        eng.constraint_store_reserve(8, 8)
        mid = eng.upload_map(8, 8, OBST_8)
        root = eng.search_batch([ll.LLJob(map_id=mid, algo=ll.ASTAR_EPS, start=inst["starts"][a], goal=inst["goals"][a], agent_idx=a,
                                          w=W, result_path_id=a, result_set_id=a) for a in range(n)])
        assert [r.status for r in root] == [ll.OK] * n
        paths = [[s[1:] for s in r.states] for r in root]
        jobs, flat = [], []
        for a in range(n):
            k = max(1, len(paths[a]) // 2)
            add = [[k] + paths[a][k]]
            kw = dict(map_id=mid, algo=ll.ASTAR_EPS, start=inst["starts"][a], goal=inst["goals"][a], agent_idx=a, w=W,
                      ctx_paths=paths, path_ids=[b if b != a else -1 for b in range(n)], vertex_constraints=add)
            jobs.append(ll.LLJob(result_path_id=4 + a, scan_conflicts=True, base_set_id=a, result_set_id=4 + a, **kw))
            flat.append(ll.LLJob(result_path_id=8 + a, **kw))
        res, conf = eng.search_batch_scan(jobs)
        plain = eng.search_batch(flat)
        sols = []
        for a in range(n):
            assert res[a].status == ll.OK and _fields(res[a]) == _fields(plain[a]), a
            S = list(paths)
            S[a] = [s[1:] for s in res[a].states]
            assert conf[a] == oracle_mod.conflict_scan(S), a
            sols.append(S)
        assert eng.conflict_scan(sols) == conf
    finally:
        eng.close()


def test_rejections(oracle_mod):
    from libmultirobotplanning_amd import ll
    mp = dict(dimx=8, dimy=8, obstacles=OBST_8)
    start, goal = [0, 0], [7, 6]
    eng = ll.LowLevelEngine(device=0, slots=64)
    try:
        mid = eng.upload_map(8, 8, OBST_8)
        mid2 = eng.upload_map(8, 8, OBST_8 + [[6, 6]])
        kw = dict(map_id=mid, algo=ll.ASTAR, start=start, goal=goal)
        good = ll.LLJob(vertex_constraints=[[1, 1, 0]], **kw)
        want = eng.search_batch([good])[0]
        assert want.status == ll.OK
        _vs_oracle(oracle_mod, ll, ll.ASTAR, mp, 0, start, goal, [[1, 1, 0]], [], [], 1.0, want)

        def statuses(jobs, **args):
            res = eng.wait_sets(eng.submit_sets([good] + list(jobs) + [good], **args))[0]
            assert _fields(res[0]) == _fields(want) and _fields(res[-1]) == _fields(want)  # the other jobs of the call
            return [r.status for r in res[1:-1]]

        # no store reserved
        assert statuses([ll.LLJob(result_set_id=0, **kw)]) == [ll.BAD_JOB]
        eng.constraint_store_reserve(8, 4)
        base = eng.search_batch([ll.LLJob(vertex_constraints=[[1, 1, 0]], result_set_id=0, **kw)])[0]
        assert _fields(base) == _fields(want)
        bad = [
            ll.LLJob(base_set_id=8, **kw), ll.LLJob(result_set_id=8, **kw), ll.LLJob(base_set_id=0, result_set_id=99, **kw),  # ids
            ll.LLJob(base_set_id=5, result_set_id=6, **kw),                                   # the base was never written
            ll.LLJob(base_set_id=0, result_set_id=6, **dict(kw, map_id=mid2)),                # another map
            ll.LLJob(base_set_id=0, result_set_id=6, **dict(kw, goal=[6, 7])),                # another goal cell
            ll.LLJob(base_set_id=0, result_set_id=0, **kw),                                   # base == result
            ll.LLJob(base_set_id=0, result_set_id=6, vertex_constraints=[[t, 4, 4] for t in range(1, 5)], **kw),  # 1 + 4 words > 4
            ll.LLJob(base_set_id=0, result_set_id=6, **dict(kw, algo=ll.ASTAR_TA, goal=None)),  # not A* / A*-epsilon
        ]
        assert statuses(bad) == [ll.BAD_JOB] * len(bad)
        # a root chain (the flag goes into the marshalled job: the wrapper has no field for it)
        import ctypes
        chain = [good, ll.LLJob(base_set_id=0, result_set_id=6, **dict(kw, algo=ll.ASTAR_EPS)), good]
        cjobs, cres, (keep, states, actions, costs) = eng._marshal(chain, eng.max_horizon)
        cjobs[1].flags |= ll.JOB_ROOT_CHAIN
        refs = (ll.mrp_ll_constraint_ref * 3)()
        for i, j in enumerate(chain):
            refs[i].base_set_id, refs[i].result_set_id = j.base_set_id, j.result_set_id
        ticket = ctypes.c_int32(-1)
        assert eng._lib.mrp_ll_submit_sets(eng._h, 0, 3, cjobs, cres, None, refs, ctypes.byref(ticket)) == 0
        assert eng._lib.mrp_ll_wait(eng._h, ticket.value) == 0
        res = eng._results(3, eng.max_horizon, cres, states, actions, costs)
        assert res[1].status == ll.BAD_JOB and _fields(res[0]) == _fields(want) and _fields(res[2]) == _fields(want)
        # none of the rejected jobs created set 6 (or changed set 0)
        assert statuses([ll.LLJob(base_set_id=6, **kw)]) == [ll.BAD_JOB]
        assert statuses([ll.LLJob(base_set_id=0, **kw)]) == [ll.OK]
        # the writer's ticket has not been collected yet
        h1 = eng.submit_sets([ll.LLJob(base_set_id=0, result_set_id=1, **kw)])
        h2 = eng.submit_sets([ll.LLJob(base_set_id=1, result_set_id=2, **kw), ll.LLJob(base_set_id=0, **kw)])
        assert eng.wait_sets(h1)[0][0].status == ll.OK
        assert [r.status for r in eng.wait_sets(h2)[0]] == [ll.BAD_JOB, ll.OK]
        assert statuses([ll.LLJob(base_set_id=1, result_set_id=2, **kw)]) == [ll.OK]  # ... and now it has
        assert statuses([ll.LLJob(base_set_id=2, **kw)]) == [ll.OK]
        # a flagged job through any other entry point: mrp_ll_search_batch (mrp_ll_submit) and mrp_ll_submit_scan
        flagged = [ll.LLJob(base_set_id=0, **kw), good]
        cjobs, cres, (keep, states, actions, costs) = eng._marshal(flagged, eng.max_horizon)
        assert eng._lib.mrp_ll_search_batch(eng._h, 2, cjobs, cres) == 0
        res = eng._results(2, eng.max_horizon, cres, states, actions, costs)
        assert res[0].status == ll.BAD_JOB and _fields(res[1]) == _fields(want)
        conf = (ll.mrp_ll_conflict * 2)()
        assert eng._lib.mrp_ll_submit_scan(eng._h, 0, 2, cjobs, cres, conf, ctypes.byref(ticket)) == 0
        assert eng._lib.mrp_ll_wait(eng._h, ticket.value) == 0
        res = eng._results(2, eng.max_horizon, cres, states, actions, costs)
        assert res[0].status == ll.BAD_JOB and _fields(res[1]) == _fields(want)
        # unflagged jobs through mrp_ll_submit_sets with sets == NULL (and conflicts == NULL) behave as through mrp_ll_submit
        cjobs, cres, (keep, states, actions, costs) = eng._marshal([good, good], eng.max_horizon)
        assert eng._lib.mrp_ll_submit_sets(eng._h, 0, 2, cjobs, cres, None, None, ctypes.byref(ticket)) == 0
        assert eng._lib.mrp_ll_wait(eng._h, ticket.value) == 0
        for r in eng._results(2, eng.max_horizon, cres, states, actions, costs):
            assert _fields(r) == _fields(want)
        # a duplicate addition costs a word and changes no result
        dup = eng.search_batch([ll.LLJob(vertex_constraints=[[1, 1, 0]], base_set_id=0, result_set_id=3, **kw)])[0]
        assert _fields(dup) == _fields(want)
        again = eng.search_batch([ll.LLJob(base_set_id=3, **kw)])[0]
        assert _fields(again) == _fields(want)
        # release_maps forgets every set
        eng.release_maps()
        mid = eng.upload_map(8, 8, OBST_8)
        assert statuses([ll.LLJob(base_set_id=0, **dict(kw, map_id=mid))]) == [ll.BAD_JOB]
        # words_per_slot beyond the copy area
        with pytest.raises(RuntimeError):
            eng.constraint_store_reserve(4, 2049)
    finally:
        eng.close()


def test_the_words_stay_on_the_device(oracle_mod):
    """In a session (where staged_bytes counts what the host writes for the device to read): a by-set job at depth 40 stages
    exactly what a by-set job at depth 1 stages, and less than the flat job at depth 40."""
    from libmultirobotplanning_amd import ll
    mp = MAPS["8x8"]
    rng = random.Random(5)
    free = _free_cells(mp)
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        eng.constraint_store_reserve(3, 64)
        mid = eng.upload_map(8, 8, mp["obstacles"])
        kw = dict(map_id=mid, algo=ll.ASTAR, start=mp["start"], goal=mp["goal"])
        eng.session_begin(64)
        try:
            def staged(job):
                eng.reset_stats()
                r = eng.search_batch([job])[0]
                return eng.stats()["staged_bytes"], r

            cons = [_random_vertex(rng, free) for _ in range(40)]
            depth1, _ = staged(ll.LLJob(vertex_constraints=cons[:1], result_set_id=1, **kw))
            for d in range(2, 40):
                eng.search_batch([ll.LLJob(vertex_constraints=cons[d - 1:d], base_set_id=(d - 1) % 3, result_set_id=d % 3, **kw)])
            depth40, r = staged(ll.LLJob(vertex_constraints=cons[39:40], base_set_id=39 % 3, result_set_id=40 % 3, **kw))
            flat40, f = staged(ll.LLJob(vertex_constraints=cons, **kw))
            assert _fields(r) == _fields(f)
            _vs_oracle(oracle_mod, ll, ll.ASTAR, mp, 0, mp["start"], mp["goal"], cons, [], [], 1.0, r)
            assert depth40 == depth1 > 0
            assert flat40 == depth40 + 4 * 39
        finally:
            eng.session_end()
    finally:
        eng.close()
