"""One collection routine, three ways to reach it: the same eight jobs collected through batch mrp_ll_submit + mrp_ll_wait,
through a mixed session with mrp_ll_submit + mrp_ll_poll, and through a mixed session with mrp_ll_submit_tagged +
mrp_ll_poll_any_tagged.  Status, cost, fmin, states and actions must be the same each time and equal to the oracle's, and
the engine's job counter must advance by the seven searches that ran (a job rejected on the host is none)."""
import ctypes
import time

import pytest

pytestmark = pytest.mark.gpu

DIM = 8
OBST = [[3, 3], [3, 4], [4, 3], [5, 6]]


def _cases(ll, oracle_mod):
    """(LLJob keyword arguments, oracle result or None for the job the host rejects)."""
    m = dict(dimx=DIM, dimy=DIM, obstacles=OBST)
    p1 = [[0, 7], [1, 7], [2, 7], [3, 7], [4, 7]]
    p2 = [[7, 0], [6, 0], [5, 0]]
    vc = [[2, 2, 0], [3, 1, 1], [9, 7, 7]]
    ec = [[0, 0, 0, 1, 0]]
    A, E = oracle_mod.ASTAR, oracle_mod.ECBS
    out = [
        (dict(algo=ll.ASTAR, start=[0, 0], goal=[7, 7], vertex_constraints=vc, edge_constraints=ec, initial_cost=5),
         oracle_mod.ll_search(A, m, 0, [0, 0], [7, 7], vertex_constraints=vc, edge_constraints=ec, initial_cost=5)),
        (dict(algo=ll.ASTAR_EPS, start=[0, 6], goal=[6, 7], w=1.5, agent_idx=0, ctx_paths=[[], p1, p2]),
         oracle_mod.ll_search(E, m, 0, [0, 6], [6, 7], ctx_paths=[[], p1, p2], w=1.5)),
        (dict(algo=ll.ASTAR_EPS, start=[7, 1], goal=[2, 0], w=1.3, agent_idx=2, vertex_constraints=[[1, 6, 1]],
              ctx_paths=[p1, p2, []]),
         oracle_mod.ll_search(E, m, 2, [7, 1], [2, 0], vertex_constraints=[[1, 6, 1]], ctx_paths=[p1, p2, []], w=1.3)),
        (dict(algo=ll.ASTAR, start=[DIM, 0], goal=[1, 1]), None),  # start outside the grid: rejected on the host
        (dict(algo=ll.ASTAR_TA, start=[2, 2], goal=None, vertex_constraints=[[0, 2, 2], [2, 2, 3], [4, 1, 1]]),
         oracle_mod.ta_ll_search(m, [2, 2], None, vertex_constraints=[[0, 2, 2], [2, 2, 3], [4, 1, 1]])),
        (dict(algo=ll.ASTAR, start=[0, 0], goal=[7, 7], max_expansions=1),
         oracle_mod.ll_search(A, m, 0, [0, 0], [7, 7], cap_expansions=1)),
        (dict(algo=ll.ASTAR, start=[7, 0], goal=[0, 7]), oracle_mod.ll_search(A, m, 0, [7, 0], [0, 7])),
        (dict(algo=ll.ASTAR_EPS, start=[4, 4], goal=[2, 2], w=1.2), oracle_mod.ll_search(E, m, 0, [4, 4], [2, 2], w=1.2)),
    ]
    assert out[5][1]["rc"] == -1 and all(o["success"] for k, (_, o) in enumerate(out) if k not in (3, 5))
    return out


def _digest(results):
    return [(r.status, r.cost, r.fmin, r.states, r.actions) for r in results]


def _until(deadline_s, step):
    t0 = time.monotonic()
    while not step():
        assert time.monotonic() - t0 < deadline_s, "no completion within %d s" % deadline_s


def test_batch_poll_and_tagged_collection_agree(oracle_mod):
    from libmultirobotplanning_amd import ll
    I32P = ctypes.POINTER(ctypes.c_int32)
    cases = _cases(ll, oracle_mod)
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=32)
    lib, h = eng._lib, eng._h
    lib.mrp_ll_submit_tagged.restype = ctypes.c_int
    lib.mrp_ll_submit_tagged.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ll.mrp_ll_job),
                                         ctypes.POINTER(ll.mrp_ll_result), I32P]
    lib.mrp_ll_poll_any_tagged.restype = ctypes.c_int
    lib.mrp_ll_poll_any_tagged.argtypes = [ctypes.c_void_p, ctypes.c_int32, I32P, ctypes.c_int32, I32P]
    try:
        mid = eng.upload_map(DIM, DIM, OBST)
        jobs = [ll.LLJob(map_id=mid, **kw) for kw, _ in cases]
        n, cap = len(jobs), eng.max_horizon
        assert n == 8

        def run(submit, collect):
            jobs0 = eng.stats()["jobs"]
            cjobs, cres, (keep, states, actions, costs) = eng._marshal(jobs, cap)
            ticket = ctypes.c_int32(-1)
            eng._check(submit(cjobs, cres, ctypes.byref(ticket)), "submit")
            collect(ticket.value)
            res = eng._results(n, cap, cres, states, actions, costs)
            assert eng.stats()["jobs"] - jobs0 == 7  # the rejected job is not counted
            return res

        def wait(ticket):
            eng._check(lib.mrp_ll_wait(h, ticket), "mrp_ll_wait")

        def poll(ticket):
            done = ctypes.c_int32(0)

            def step():
                eng._check(lib.mrp_ll_poll(h, ticket, ctypes.byref(done)), "mrp_ll_poll")
                return done.value == 1
            _until(60, step)

        def poll_any_tagged(ticket):
            got, cnt = (ctypes.c_int32 * 4)(), ctypes.c_int32(0)
            seen = []

            def step():
                eng._check(lib.mrp_ll_poll_any_tagged(h, 1, got, 4, ctypes.byref(cnt)), "mrp_ll_poll_any_tagged")
                seen.extend(got[k] for k in range(cnt.value))
                return bool(seen)
            _until(60, step)
            assert seen == [ticket]

        batch = run(lambda cj, cr, t: lib.mrp_ll_submit(h, n, cj, cr, t), wait)
        eng.session_begin(16)
        try:
            polled = run(lambda cj, cr, t: lib.mrp_ll_submit(h, n, cj, cr, t), poll)
        finally:
            eng.session_end()
        eng.session_begin(16)
        try:
            tagged = run(lambda cj, cr, t: lib.mrp_ll_submit_tagged(h, 1, n, cj, cr, t), poll_any_tagged)
        finally:
            eng.session_end()
    finally:
        eng.close()

    assert _digest(batch) == _digest(polled) == _digest(tagged)
    for k, ((_, o), r) in enumerate(zip(cases, batch)):
        if o is None:
            assert (r.status, r.n_states) == (ll.BAD_JOB, 0), k
        elif o["rc"] == -1:
            assert r.status == ll.CAP_EXPANSIONS, k
        else:
            assert r.status == ll.OK, (k, r.status)
            assert (r.cost, r.fmin, r.expanded, r.states, r.actions) == (o["cost"], o["fmin"], o["expanded"], o["states"],
                                                                         o["actions"]), k
            if "action_costs" in o:
                assert r.action_costs == o["action_costs"], k
