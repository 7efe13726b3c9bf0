"""The select-address stores of the expansion's heap steps and the straight-line top of the search loop (ll_compact.h
ldsStoreSel, compactSearch's one sign test for all of its exits) on the MI355X: the searches of tests/loop_exit_cases.py and
tests/push_cases.py as ordinary jobs of a front / heavy session with mrp_ll_session_front_tables on — the front workgroups run
compactSearch<true, false, true> (narrow), the heavy ones the wide instance — with their context shipped, once more with
MRP_LL_JOB_HEAVY; as a batch of the A*-epsilon kernel and, without the context, of the A* kernel; and a ten-agent root
chain.  Status, cost, fmin, n_states, expanded, states and tier are compared with the oracle; integers, exact.

The engine runs a job to its end: a case of loop_exit_cases.py that leaves the narrow tier under the emulator's tight limits
(over_open, over_t) stays inside it here, and the one whose focalH outgrows the narrow entry (over_fh) is handed over and
finishes with the oracle's answer in another tier."""
import pytest

import loop_exit_cases as lx
import oracle
import push_cases as pc
import root_chain_cases as rc
import test_root_chain_gpu as rcg
from test_front_tables_gpu import FrontWorld

pytestmark = pytest.mark.gpu

TIER_FRONT, TIER_HEAVY = 0, 2  # include/mrp_ll.h mrp_ll_result.tier
OK, NO_SOLUTION, CAP_EXPANSIONS = 0, 1, 2
WORDS = ("status", "cost", "fmin", "n_states", "expanded")


def _cases():
    """(name, case, max_expansions, leaves the front tier): loop_exit_cases.py's (one of the two over_fh: they are one search)
    and push_cases.py's."""
    out = [(c["name"], c, c["max_exp"], c["name"].startswith("over_fh")) for c in lx.cases() if c["name"] != "over_fh_wide"]
    return out + [(c["name"], c, -1, False) for c in pc.cases()]


def _want(c, algo, max_exp):
    """The oracle's words for the case under `algo` (A*: no context, w = 1)."""
    eps = algo == oracle.ECBS
    o = oracle.ll_search(algo, c["inst"], c["agent"], c["inst"]["starts"][c["agent"]], c["inst"]["goals"][c["agent"]],
                         vertex_constraints=c["vc"], edge_constraints=c["ec"], ctx_paths=c["ctx_paths"] if eps else [],
                         w=lx.W if eps else 1.0, cap_expansions=max_exp)
    if o["rc"] == -1:  # the cap: the pop that passed it is counted
        return dict(status=CAP_EXPANSIONS, expanded=max_exp + 1)
    if not o["success"]:
        return dict(status=NO_SOLUTION, expanded=o["expanded"])
    return dict(status=OK, cost=o["cost"], fmin=o["fmin"], n_states=len(o["states"]), expanded=o["expanded"],
                states=[list(s) for s in o["states"]])


def _diff(r, want):
    got = dict(status=r.status, cost=r.cost, fmin=r.fmin, n_states=r.n_states, expanded=r.expanded,
               states=[list(s) for s in r.states])
    return {k: (got[k], v) for k, v in want.items() if got[k] != v}


@pytest.fixture(scope="module")
def world(oracle_mod):
    from libmultirobotplanning_amd import ll
    w = FrontWorld(ll)
    try:
        w.eng.path_store_reserve(16)
        w.chain_case = next(c for c in rc.select_cases() if len(c["inst"]["starts"]) == 10 and c["w"] == 1.3)
        for inst in [c["inst"] for _, c, _, _ in _cases()] + [w.chain_case["inst"]]:  # every map before the first session
            w.map_of(inst)
        w.want = {algo: {name: _want(c, algo, cap) for name, c, cap, _ in _cases()} for algo in (oracle.ECBS, oracle.ASTAR)}
        yield w
        assert w.eng.stats()["heavy_fallbacks"] == 0
    finally:
        w.eng.close()


def _jobs(world, algo, heavy=False):
    ll = world.ll
    eps = algo == ll.ASTAR_EPS
    return [ll.LLJob(map_id=world.map_of(c["inst"]), algo=algo, start=c["inst"]["starts"][c["agent"]],
                     goal=c["inst"]["goals"][c["agent"]], agent_idx=c["agent"], w=lx.W if eps else 1.0, vertex_constraints=c["vc"],
                     edge_constraints=c["ec"], ctx_paths=c["ctx_paths"] if eps else [], max_expansions=cap, heavy=heavy)
            for _, c, cap, _ in _cases()]


@pytest.mark.parametrize("heavy", [False, True], ids=["front", "heavy"])
def test_session_jobs_equal_the_oracle(world, heavy):
    with world.session():
        res = world.eng.search_batch(_jobs(world, world.ll.ASTAR_EPS, heavy))
    bad = []
    for (name, _, _, leaves), r in zip(_cases(), res):
        d = _diff(r, world.want[oracle.ECBS][name])
        print(name, "heavy" if heavy else "front", "tier", r.tier, {k: getattr(r, k) for k in WORDS})
        if d or (r.tier != (TIER_HEAVY if heavy else TIER_FRONT) and not leaves) or (leaves and not heavy and r.tier == TIER_FRONT):
            bad.append((name, r.tier, d))
    assert not bad, bad
    assert world.eng.stats()["heavy_fallbacks"] == 0


@pytest.mark.parametrize("algo", ["astar_eps", "astar"])
def test_batch_jobs_equal_the_oracle(world, algo):
    """No session: one launch of the batch kernel of the algorithm (A*: the same maps and constraints without the context)."""
    ll_algo, ref = (world.ll.ASTAR_EPS, oracle.ECBS) if algo == "astar_eps" else (world.ll.ASTAR, oracle.ASTAR)
    res = world.eng.search_batch(_jobs(world, ll_algo))
    bad = []
    for (name, _, _, _), r in zip(_cases(), res):
        d = _diff(r, world.want[ref][name])
        print(name, algo, "tier", r.tier, {k: getattr(r, k) for k in WORDS})
        if d:
            bad.append((name, r.tier, d))
    assert not bad, bad


def test_a_ten_agent_root_chain(world):
    """Every search of the chain pops, erases and pushes through the select-address stores and leaves through the goal block."""
    inst, model = world.chain_case["inst"], world.chain_case["model"]
    b = rc.Batch()
    b.add_chain(world.map_of(inst), inst, 1.3, list(range(10)))
    with world.session():
        (got,) = world.run(b)
    assert rcg._chain_diff(got, model) == []
    assert world.eng.stats()["heavy_fallbacks"] == 0
