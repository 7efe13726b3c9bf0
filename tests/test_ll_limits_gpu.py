"""The arena-tier searches on large and non-square maps and at their loud limits, on the MI355X: the corpus of
tests/limit_cases.py through the C-ABI.  A case the reference proves to be inside the documented limits (include/mrp_ll.h)
must come back bit for bit — status, cost, fmin, expansions, states, actions; one it proves to be beyond exactly one limit must
come back with that limit's status (MRP_LL_CAP_NODES / _HORIZON / _FOCAL) and without a path; the few cases with no proof
either way may be exact or report CAP_NODES / CAP_HORIZON, nothing else.  A key field that wraps instead of reporting — g at
1024, h at 2048, focalH at 2048 — yields a plausible wrong path and fails here."""
import collections

import pytest

import limit_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    return lc.corpus()


@pytest.fixture(scope="module")
def engines():
    """name -> state of the engine with the option set lc.ENGINES[name], created on first use (at most four in this module),
    every one closed when the module is done.  state: eng, maps / heurs (what has been uploaded), batch (name -> result)."""
    from libmultirobotplanning_amd import ll
    made = {}

    def get(name):
        if name not in made:
            made[name] = dict(eng=ll.LowLevelEngine(device=0, **lc.ENGINES[name]), maps={}, heurs={}, batch={})
        return made[name]
    try:
        yield get
    finally:
        for st in made.values():
            st["eng"].close()


def _jobs(st, cases):
    from libmultirobotplanning_amd import ll
    eng, maps, heurs = st["eng"], st["maps"], st["heurs"]
    algo_id = dict(astar=ll.ASTAR, eps=ll.ASTAR_EPS, ta=ll.ASTAR_TA, eps_ta=ll.ASTAR_EPS_TA)
    jobs = []
    for c in cases:
        m, g = c["map"], c["goal"]
        if id(m) not in maps:
            maps[id(m)] = eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        hid = -1
        if g is not None and c["algo"] in ("ta", "eps_ta"):
            hk = (id(m), tuple(g), c["heur"])
            if hk not in heurs:
                heurs[hk] = eng.compute_heuristics([maps[id(m)]], [g])[0] if c["heur"] == "device" else \
                    eng.upload_heuristic(maps[id(m)], lc.table(m, g))
            hid = heurs[hk]
        jobs.append(ll.LLJob(map_id=maps[id(m)], algo=algo_id[c["algo"]], start=c["start"], goal=g, agent_idx=c["agent"],
                             w=c["w"], vertex_constraints=c["vc"], edge_constraints=c["ec"], ctx_paths=c["ctx"], heuristic_id=hid))
    return jobs


def _key(r):
    return (r.status, r.cost, r.fmin, r.expanded, r.n_states, r.states, r.actions, r.action_costs)


def _check(cases, res, arena):
    """The class assertions of the module docstring.  Returns the class counts."""
    from libmultirobotplanning_amd import ll
    caps = (ll.CAP_NODES, ll.CAP_HORIZON, ll.CAP_FOCAL)
    seen = collections.Counter()
    assert len(res) == len(cases)
    for c, r in zip(cases, res):
        o = c["ref"]
        tag = (c["name"], c["cls"], c["expect"], c["why"], "status", r.status, "expanded", r.expanded, o["expanded"])
        if r.status in caps:
            assert r.n_states == 0 and r.states == [] and r.actions == [], tag  # never a path next to a capacity status
        if arena:
            assert r.tier == 1, tag
        exact = False
        if c["cls"] == "outside":
            assert r.status == getattr(ll, c["expect"]), tag
        elif c["cls"] == "between":
            exact = r.status not in (ll.CAP_NODES, ll.CAP_HORIZON)
        else:
            exact = True
        if exact:
            assert r.status == (ll.OK if o["success"] else ll.NO_SOLUTION), tag
            assert r.expanded == o["expanded"], tag
            if o["success"]:
                assert (r.cost, r.fmin, r.n_states) == (o["cost"], o["fmin"], len(o["states"])), (tag, r.cost, r.fmin, o["cost"], o["fmin"])
                assert r.states == o["states"] and r.actions == o["actions"], tag
                if "action_costs" in o:
                    assert r.action_costs == o["action_costs"], tag
        seen[(c["algo"], c["cls"], c["expect"])] += 1
    return seen


def _batch(engines, corpus, name):
    st = engines(name)
    if "all" not in st["batch"]:
        cases = [c for c in corpus if c["engine"] == name]
        st["batch"]["all"] = (cases, st["eng"].search_batch(_jobs(st, cases), states_cap=lc.ENGINES[name]["max_horizon"]))
    return st["batch"]["all"]


def test_large_and_non_square_maps(engines, corpus):
    """33 x 31 to 255 x 255 (one row, one column and three rows of 255 among them), default arena and horizon: all four
    algorithms in the arena tier, constraints on the last row, the last column and cell (254, 254) up to time 511, edge
    constraints that leave the grid, context paths along the last row and column.  On 255 x 255 the task-assignment
    searches have 8 and 10 time steps: cases inside and outside them."""
    cases, res = _batch(engines, corpus, "big")
    seen = _check(cases, res, arena=True)
    for algo in lc.ALGOS:
        assert seen[(algo, "inside", None)] >= 100, seen
    assert seen[("ta", "outside", "CAP_HORIZON")] >= 4 and seen[("eps_ta", "outside", "CAP_HORIZON")] >= 2, seen


def test_arena_tier_on_small_maps_and_the_node_and_focal_limits(engines, corpus):
    """An engine without the LDS tier and with 4096 arena nodes: 31 x 17, 17 x 31, 32 x 5, 1 x 32 and 1 x 1 in the arena
    tier; CAP_NODES on 48 x 48; the focalH cases n * L = 2047 and 2000 (exact), 2070, 2100 and 2100 (CAP_FOCAL) for
    MRP_LL_ASTAR_EPS and MRP_LL_ASTAR_EPS_TA."""
    cases, res = _batch(engines, corpus, "arena_only")
    seen = _check(cases, res, arena=True)
    assert seen[("astar", "outside", "CAP_NODES")] >= 1 and seen[("eps", "outside", "CAP_NODES")] >= 1, seen
    assert seen[("eps", "outside", "CAP_FOCAL")] == 3 and seen[("eps_ta", "outside", "CAP_FOCAL")] == 3, seen
    for algo in lc.ALGOS:
        assert seen[(algo, "inside", None)] >= 20, seen


def test_focal_limit_through_the_compact_tier(engines, corpus):
    """The same focalH cases through a default engine: the compact tier starts them, must hand them over before its own
    focalH field overflows, and the arena tier answers exactly or with CAP_FOCAL."""
    cases, res = _batch(engines, corpus, "default")
    seen = _check(cases, res, arena=False)
    assert seen[("eps", "inside", None)] == 2 and seen[("eps", "outside", "CAP_FOCAL")] == 3, seen


def test_g_horizon_f_and_h_fields(engines, corpus):
    """max_horizon 1024, 2^22 arena nodes: a goal 1022 and 1023 corridor steps away is exact (A*: 490 000 expansions), 1024
    steps are CAP_HORIZON for all four algorithms; task-assignment starts whose table value is 2044, 2046, 2078 and 4000
    are CAP_HORIZON (tables computed on the device) — an h wrapped to 11 bits would let three of them search on."""
    cases, res = _batch(engines, corpus, "long")
    seen = _check(cases, res, arena=True)
    for algo in lc.ALGOS:
        assert seen[(algo, "outside", "CAP_HORIZON")] >= 1, seen
    assert seen[("astar", "inside", None)] == 2 and seen[("eps", "inside", None)] == 1, seen
    assert seen[("ta", "outside", "CAP_HORIZON")] == 5 and seen[("eps_ta", "outside", "CAP_HORIZON")] == 5, seen


@pytest.mark.parametrize("name", ["big", "arena_only"])
def test_geometry_cases_in_a_mixed_session(engines, corpus, name):
    """The geometry cases once more through the resident mixed kernel (mrp_ll_session_begin): identical to batch mode, word
    for word (maps and heuristic tables were uploaded before the session began)."""
    cases, res = _batch(engines, corpus, name)
    pick = [i for i, c in enumerate(cases) if c["group"] == "geometry"]
    st = engines(name)
    jobs = _jobs(st, [cases[i] for i in pick])
    eng = st["eng"]
    eng.session_begin(lc.ENGINES[name]["slots"])
    try:
        got = []
        for k in range(0, len(jobs), 128):
            got += eng.search_batch(jobs[k:k + 128], states_cap=lc.ENGINES[name]["max_horizon"])
    finally:
        eng.session_end()
    assert len(got) == len(pick) >= 100
    for i, r in zip(pick, got):
        assert _key(r) == _key(res[i]), (cases[i]["name"], r.status, res[i].status, r.expanded, res[i].expanded)
