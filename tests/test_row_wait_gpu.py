"""The lane mask of the focal-table row loads on the MI355X: the searches of tests/row_wait_cases.py as ordinary jobs of a
front / heavy session with mrp_ll_session_front_tables on — the front workgroups run compactSearch<true, false, true> (narrow),
the heavy ones the wide instance — with the context shipped and named by path-store ids, once more with MRP_LL_JOB_HEAVY, and a
ten-agent root chain.  Everything is compared with the oracle; integers, exact."""
import pytest

import root_chain_cases as rc
import row_wait_cases as rw
import test_root_chain_gpu as rcg
from test_front_tables_gpu import FRONT_WGS, HEAVY_WGS, FrontWorld

pytestmark = pytest.mark.gpu

TIER_FRONT, TIER_HEAVY = 0, 2  # include/mrp_ll.h mrp_ll_result.tier


@pytest.fixture(scope="module")
def world(oracle_mod):
    """The engine, the cases' one map, and the context paths of every case in the path store (slot0[name] + agent): each
    context agent planned alone by the engine, which must find the path the oracle found."""
    from libmultirobotplanning_amd import ll
    w = FrontWorld(ll)
    try:
        cases = rw.cases()
        w.chain_slot0 = sum(c["n"] for c in cases)
        w.eng.path_store_reserve(w.chain_slot0 + 10)
        w.mid = w.map_of(cases[0]["inst"])
        w.chain_case = next(c for c in rc.select_cases() if len(c["inst"]["starts"]) == 10 and c["w"] == 1.3)
        w.map_of(w.chain_case["inst"])  # (every map before the first session)
        w.slot0, nxt, alone = {}, 0, []
        for c in cases:
            w.slot0[c["name"]] = nxt
            for a in range(1, c["n"]):
                alone.append((c, a, ll.LLJob(map_id=w.mid, algo=ll.ASTAR_EPS, start=c["inst"]["starts"][a], goal=c["inst"]["goals"][a],
                                             agent_idx=a, w=rw.W, result_path_id=nxt + a)))
            nxt += c["n"]
        res = w.eng.search_batch([j for _, _, j in alone])
        for (c, a, _), r in zip(alone, res):
            assert r.status == ll.OK and [s[1:] for s in r.states] == c["ctx_paths"][a], (c["name"], a)
        yield w
        assert w.eng.stats()["heavy_fallbacks"] == 0
    finally:
        w.eng.close()


def _jobs(w, by_id, heavy):
    ll = w.ll
    out = []
    for c in rw.cases():
        kw = dict(map_id=w.mid, algo=ll.ASTAR_EPS, start=c["inst"]["starts"][0], goal=c["inst"]["goals"][0], agent_idx=0, w=rw.W,
                  vertex_constraints=c["vc"], edge_constraints=c["ec"], ctx_paths=c["ctx_paths"], heavy=heavy)
        if by_id:
            kw["path_ids"] = [-1] + [w.slot0[c["name"]] + a for a in range(1, c["n"])]
        out.append(ll.LLJob(**kw))
    return out


@pytest.mark.parametrize("form,heavy", [("shipped", False), ("ids", False), ("ids", True)], ids=["shipped", "ids", "ids_heavy"])
def test_jobs_equal_the_oracle(world, form, heavy):
    with world.session():
        res = world.eng.search_batch(_jobs(world, form == "ids", heavy))
    bad = []
    for c, r in zip(rw.cases(), res):
        want = rw.expected(c)
        got = dict(status=r.status, cost=r.cost, fmin=r.fmin, n_states=r.n_states, expanded=r.expanded,
                   states=[list(s) for s in r.states])
        print(c["name"], form, "heavy" if heavy else "", "tier", r.tier, {k: got[k] for k in ("status", "cost", "fmin", "n_states", "expanded")})
        if got != want or r.tier != (TIER_HEAVY if heavy else TIER_FRONT):
            bad.append((c["name"], r.tier, got, want))
    assert not bad, bad


def test_a_ten_agent_root_chain(world):
    """The chain's own table (64 rows, 16 columns, the columns of the agents not yet planned empty)."""
    inst, model = world.chain_case["inst"], world.chain_case["model"]
    b = rc.Batch()
    b.add_chain(world.map_of(inst), inst, 1.3, list(range(world.chain_slot0, world.chain_slot0 + 10)))
    with world.session():
        (got,) = world.run(b)
    assert rcg._chain_diff(got, model) == []
