"""The expansion's push step and the heap roots kept in a register (ll_compact.h pushTurn, compactSearch's `tops`) on the
MI355X: the searches of tests/push_cases.py as ordinary jobs of a front / heavy session with mrp_ll_session_front_tables on —
the front workgroups run compactSearch<true, false, true> (narrow), the heavy ones the wide instance — with their context
shipped, once more with MRP_LL_JOB_HEAVY, and a ten-agent root chain.  Status, cost, fmin, n_states, expanded, states and tier
are compared with the oracle; integers, exact."""
import pytest

import push_cases as pc
import root_chain_cases as rc
import test_root_chain_gpu as rcg
from test_front_tables_gpu import FrontWorld

pytestmark = pytest.mark.gpu

TIER_FRONT, TIER_HEAVY = 0, 2  # include/mrp_ll.h mrp_ll_result.tier


@pytest.fixture(scope="module")
def world(oracle_mod):
    from libmultirobotplanning_amd import ll
    w = FrontWorld(ll)
    try:
        w.eng.path_store_reserve(16)
        w.chain_case = next(c for c in rc.select_cases() if len(c["inst"]["starts"]) == 10 and c["w"] == 1.3)
        for inst in [c["inst"] for c in pc.cases()] + [w.chain_case["inst"]]:  # every map before the first session
            w.map_of(inst)
        yield w
        assert w.eng.stats()["heavy_fallbacks"] == 0
    finally:
        w.eng.close()


@pytest.mark.parametrize("heavy", [False, True], ids=["front", "heavy"])
def test_jobs_equal_the_oracle(world, heavy):
    ll = world.ll
    jobs = [ll.LLJob(map_id=world.map_of(c["inst"]), algo=ll.ASTAR_EPS, start=c["inst"]["starts"][c["agent"]],
                     goal=c["inst"]["goals"][c["agent"]], agent_idx=c["agent"], w=pc.W, vertex_constraints=c["vc"],
                     edge_constraints=c["ec"], ctx_paths=c["ctx_paths"], heavy=heavy) for c in pc.cases()]
    with world.session():
        res = world.eng.search_batch(jobs)
    bad = []
    for c, r in zip(pc.cases(), res):
        want = pc.expected(c)
        got = dict(status=r.status, cost=r.cost, fmin=r.fmin, n_states=r.n_states, expanded=r.expanded,
                   states=[list(s) for s in r.states])
        print(c["name"], "heavy" if heavy else "front", "tier", r.tier, {k: got[k] for k in ("status", "cost", "fmin", "n_states", "expanded")})
        if got != want or r.tier != (TIER_HEAVY if heavy else TIER_FRONT):
            bad.append((c["name"], r.tier, got, want))
    assert not bad, bad
    assert world.eng.stats()["heavy_fallbacks"] == 0


def test_a_ten_agent_root_chain(world):
    """The chain's own table (64 rows, 16 columns): every search of the chain pushes and pops through the kept roots."""
    inst, model = world.chain_case["inst"], world.chain_case["model"]
    b = rc.Batch()
    b.add_chain(world.map_of(inst), inst, 1.3, list(range(10)))
    with world.session():
        (got,) = world.run(b)
    assert rcg._chain_diff(got, model) == []
    assert world.eng.stats()["heavy_fallbacks"] == 0
