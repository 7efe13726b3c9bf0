"""mrp_ll_session_front_tables(ctx, 1) on the MI355X: the front workgroups of a front / heavy session keep every focal path
table in their arena slot, are launched with the 10 880-byte window alone, and run the search that reads the table's two rows
with vector loads.  Nothing a caller sees may depend on it:

  * the root chains of tests/root_chain_cases.py against its model (whole chains, the path store, chunks and resumption, the
    shared budget, the break in front of a search that outgrows the tier, refused chains) — the checks of
    tests/test_root_chain_gpu.py, run here in a session of 32 front and 4 heavy workgroups with the mode on;
  * conflict-tree children that name their context by path-store ids, with and without MRP_LL_JOB_SCAN_CONFLICTS, at ten agents
    (one row load per table row) and at 65 (two), against the oracle's search and the oracle's conflict scan;
  * the ECBS session driver on a stream of batches, MRP_HL_FRONT_TABLES=memory against =lds and against the oracle;
  * the geometry the engine reports, and no fall-back to a single all-tier launch.

Every comparison is of integers and exact."""
import contextlib

import numpy as np
import pytest

import root_chain_cases as rc
import test_node_scan_gpu as nsg
import test_root_chain_gpu as rcg

pytestmark = pytest.mark.gpu

FRONT_WGS, HEAVY_WGS = 32, 4
NARROW_WINDOW = 10880  # ct::Narrow::windowBytes(true) (ll_compact.h; tests/test_node_scan_gpu.py pins the same number)
E_BUSY = -4            # include/mrp_ll.h MRP_LL_E_BUSY


class FrontWorld(rcg.World):
    """The world of tests/test_root_chain_gpu.py whose A*-epsilon sessions are front / heavy pairs with the tables in memory."""

    def __init__(self, ll):
        super().__init__(ll)
        self.eng.session_front_tables(True)

    @contextlib.contextmanager
    def session(self, mixed=False):
        if mixed:
            self.eng.session_begin(16)
        else:
            self.eng.session_begin_tiers(FRONT_WGS, HEAVY_WGS)
        try:
            yield
        finally:
            self.eng.session_end()


@pytest.fixture(scope="module")
def world(oracle_mod):
    from libmultirobotplanning_amd import ll
    w = FrontWorld(ll)
    try:
        w.eng.path_store_reserve(rcg.NSLOTS)
        for c in rc.select_cases():  # every map before the first session
            w.map_of(c["inst"])
        for inst in (rc.break_case()[0], rcg._filler(1), rcg.PASS, rcg.WIDE):
            w.map_of(inst)
        yield w
        assert w.eng.stats()["heavy_fallbacks"] == 0  # every session of this module ran as the pair it asked for
    finally:
        w.eng.close()


# ---- the engine's answers -------------------------------------------------------------------------------------------------

def test_geometry_follows_the_switch():
    """A new engine answers as before (tests/test_node_scan_gpu.py pins it); with the switch on the front window is the narrow
    window alone and the runtime grants at least as many front workgroups per CU; the heavy window and
    mrp_ll_session_occupancy do not move; the call is refused while a session runs, and switching back restores the answers."""
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, slots=64)
    try:
        occ0, front0, heavy0 = eng.session_tiers_geometry()
        eps0 = eng.session_occupancy(ll.ASTAR_EPS)
        assert front0 == NARROW_WINDOW + 4096
        eng.session_front_tables(True)
        occ1, front1, heavy1 = eng.session_tiers_geometry()
        print("front workgroups per CU: %d with %d bytes, %d with %d bytes" % (occ0, front0, occ1, front1))
        assert (front1, heavy1) == (NARROW_WINDOW, heavy0)
        assert occ1 >= occ0 and occ1 >= 1
        assert eng.session_occupancy(ll.ASTAR_EPS) == eps0
        eng.session_begin_tiers(FRONT_WGS, HEAVY_WGS)
        try:
            assert eng._lib.mrp_ll_session_front_tables(eng._h, 0) == E_BUSY
        finally:
            eng.session_end()
        assert eng.session_tiers_geometry() == (occ1, front1, heavy1)
        eng.session_front_tables(False)
        assert eng.session_tiers_geometry() == (occ0, front0, heavy0)
        assert eng.stats()["heavy_fallbacks"] == 0
    finally:
        eng.close()


# ---- root chains ------------------------------------------------------------------------------------------------------------

def test_whole_chains_equal_the_model_and_ordinary_jobs(world):
    """Every selected chain from agent 0 in one ticket and every agent of every chain as an ordinary job with the model's
    earlier paths shipped (a shipped table: it goes to the arena slot as well) in a second: both equal the model, field by
    field, the job's conflict count and first conflict included (the root scan reads the table from where it now is)."""
    cases = rc.select_cases()
    chains, jobs, slots, first_job = rc.Batch(), rc.Batch(), rcg.Slots(), []
    for c in cases:
        inst, n, mid = c["inst"], len(c["inst"]["starts"]), world.map_of(c["inst"])
        chains.add_chain(mid, inst, c["w"], slots.take(n))
        first_job.append(len(jobs.specs))
        for a in range(n):
            jobs.add_job(mid, inst, c["w"], a, ctx_paths=rcg._ctx_before(c["model"]["paths"], a))
    with world.session():
        t1, t2 = world.submit(chains), world.submit(jobs)
        world.collect(t1)
        world.collect(t2)
    bad = []
    for i, (c, f) in enumerate(zip(cases, first_job)):
        g = chains.result(i)
        d = rcg._chain_diff(g, c["model"])
        if d:
            bad.append((c["name"], c["cls"], d))
        for a in range(len(c["inst"]["starts"])):
            assert g["chain"][a] == jobs.result(f + a), (c["name"], a)
    assert not bad, bad
    assert {c["cls"] for c in cases} >= set(rc.CLASSES)  # roots without a conflict, with a vertex, an edge, both


def test_the_path_store_holds_the_chains_paths(world, oracle_mod):
    rcg.test_the_path_store_holds_the_chains_paths(world, oracle_mod)


def test_chunks_and_resumption(world):
    rcg.test_chunks_and_resumption(world)


def test_the_shared_budget(world):
    rcg.test_the_shared_budget(world)


def test_the_chain_ends_in_front_of_a_search_that_outgrows_the_tier(world, oracle_mod):
    rcg.test_the_chain_ends_in_front_of_a_search_that_outgrows_the_tier(world, oracle_mod)


def test_a_rejected_chain_runs_nothing_and_touches_no_slot(world, oracle_mod):
    rcg.test_a_rejected_chain_runs_nothing_and_touches_no_slot(world, oracle_mod)


# ---- wide roots: the root scan stages the table from memory, in one pass up to 64 agents and in two at 128 ---------------

def _wide_root(n, pair):
    """n agents on a 32 x 32 map, w = 1.0 (every search expands its optimal paths alone).  Agents 0 .. n - 3 stand in rows of 32
    at y = 0, 8, 16, 24 and walk 1 .. 5 steps up their own column: nobody meets anybody — except agent pair[1], whose goal is
    its left neighbour pair[0]'s (one step up): it arrives at t = 2 on a cell that is taken for good, a vertex conflict at
    every time step from there on.  The last two agents use a corridor one cell wide — row 31 below a wall along row 30, then
    up column 31 beside a wall — : agent n - 2 parks in it at (31, 30), agent n - 1 walks all of it, 34 steps, and has to pass
    that cell at t = 32.  The root's paths are up to 35 states long, so the scan covers time steps on both sides of row 31."""
    starts = [[i % 32, 8 * (i // 32)] for i in range(n - 2)] + [[31, 29], [0, 31]]
    goals = [[i % 32, 8 * (i // 32) + 1 + (i % 5)] for i in range(n - 2)] + [[31, 30], [31, 28]]
    assert pair[0] % 5 == 0 and pair[1] == pair[0] + 1 < n - 2
    goals[pair[1]] = list(goals[pair[0]])
    obstacles = [[x, 30] for x in range(31)] + [[30, 29], [30, 28]]
    return dict(dimx=32, dimy=32, obstacles=obstacles, starts=starts, goals=goals)


@pytest.mark.parametrize("n,pair", [(64, (5, 6)), (65, (5, 6)), (128, (100, 101))])
def test_wide_roots_scan_from_memory(oracle_mod, n, pair):
    """64 agents: the 8 KB table comes into the window in one piece; 65: 51 rows of 160 bytes at a time; 128: two passes of 32
    rows, the second of which holds the corridor's conflict at t = 32.  Count and first conflict are the oracle's."""
    from libmultirobotplanning_amd import ll
    inst = _wide_root(n, pair)
    model = rc.chain_model(inst, 1.0)
    scan = oracle_mod.conflict_scan(model["paths"])
    assert model["n_states"] == n and len(model["paths"][n - 1]) == 35
    assert (scan["time"], scan["type"], scan["agent1"], scan["agent2"]) == (2, 0) + pair and model["cost"] >= 31
    assert model["paths"][n - 1][32] == [31, 30] == model["paths"][n - 2][-1]  # the late conflict is in the model's root
    w = FrontWorld(ll)
    try:
        w.eng.path_store_reserve(256)
        mid = w.map_of(inst)
        b = rc.Batch()
        b.add_chain(mid, inst, 1.0, list(range(n)))
        with w.session():
            (got,) = w.run(b)
        print("n = %d: count %d first %#x" % (n, got["cost"], got["fmin"] & 0xFFFFFFFF))
        assert rcg._chain_diff(got, model) == [], (got["cost"], got["fmin"], model["cost"], model["fmin"])
        assert w.eng.stats()["heavy_fallbacks"] == 0
    finally:
        w.eng.close()


# ---- children by path-store id ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,n_agents,obstacles,seed", [(8, 10, nsg.OBST_8, 5), (32, 65, [], 6)])
def test_children_by_id_with_and_without_the_scan(oracle_mod, dim, n_agents, obstacles, seed):
    """One child job per agent of a node whose paths are in the path store, flagged and not flagged, in a front / heavy session
    with the mode on: the search is the oracle's (status, cost, fmin, expansions, states) and the conflicts are the oracle's
    scan of the node (tests/test_node_scan_gpu.py _check_node also compares the engine's own scan kernel and the two forms of
    the job with each other)."""
    from libmultirobotplanning_amd import ll
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64)
    try:
        eng.path_store_reserve(1024)
        eng.session_front_tables(True)
        node = nsg.Node(eng, nsg._instance(dim, n_agents, obstacles, seed), late_goal_agent=2)
        eng.session_begin_tiers(FRONT_WGS, HEAVY_WGS)
        try:
            res, conf = nsg._check_node(eng, oracle_mod, node)
        finally:
            eng.session_end()
        assert eng.stats()["heavy_fallbacks"] == 0
        assert 0 in {r.tier for r in res}  # searches of the front tier
        for a in range(node.n):
            ctx = [p if b != a else [] for b, p in enumerate(node.paths)]
            want = rc.plan(node.inst, nsg.W, a, ctx, left=100000, vc=node.cons[a])
            got = dict(status=res[a].status, cost=res[a].cost, fmin=res[a].fmin, n_states=res[a].n_states,
                       expanded=res[a].expanded, states=[list(s) for s in res[a].states], actions=list(res[a].actions))
            assert rc.same(got, want) == [], (a, got, want)
    finally:
        eng.close()


# ---- the session driver -----------------------------------------------------------------------------------------------------

CAP = 200000  # low-level expansions per instance, for the engine and the oracle alike


def test_driver_stream_switch_on_equals_off_and_the_oracle(monkeypatch, oracle_mod):
    """Two batches of 256 ten-agent instances and one of 32 fifty-agent instances as one stream through hl.BatchSolver, with
    MRP_HL_FRONT_TABLES=memory and =lds: identical status, cost, both counters and schedule digest (makespan too), and equal
    to the oracle's; the engines never fell back to a single launch."""
    from libmultirobotplanning_amd import hl
    batches = [hl.generate_instances(910000, 256, 32, 32, 204, 10), hl.generate_instances(920000, 256, 32, 32, 204, 10),
               hl.generate_instances(930000, 32, 32, 32, 204, 50)]
    want = [oracle_mod.mapf_solve_batch_digest(oracle_mod.ECBS, 32, 32, b.obstacles, b.starts, b.goals, w=1.3, cap_total=CAP,
                                               n_threads=16)[:2] for b in batches]
    fields = ("status", "cost", "makespan", "hl_expanded", "ll_expanded", "schedule_digest")
    got = {}
    s = hl.BatchSolver(device=0, n_threads=2)
    try:
        for mode in ("memory", "lds"):
            monkeypatch.setenv("MRP_HL_FRONT_TABLES", mode)
            preps = [s.prepare(b, want_paths=True, path_cap=128) for b in batches]
            try:
                st = s.solve_stream(preps, algo=hl.ECBS, w=1.3, max_ll_expansions=CAP)
                got[mode] = [{k: s.result_arrays(p)[k] for k in fields} for p in preps]
            finally:
                for p in preps:
                    s.release(p)
            assert st["batches"] == 3
        assert s.ll_stats()["heavy_fallbacks"] == 0
    finally:
        s.close()
    for k, (per, digest) in enumerate(want):
        on, off = got["memory"][k], got["lds"][k]
        for f in fields:
            assert np.array_equal(on[f], off[f]), (k, f)
        solved = per[:, 0] == 1
        assert solved.sum() >= len(per) * 9 // 10
        assert np.array_equal(on["status"] == hl.SOLVED, solved), k
        assert np.array_equal((on["status"] == hl.CAP), per[:, 0] == -1), k
        for f, col in (("cost", 1), ("makespan", 2), ("hl_expanded", 3), ("ll_expanded", 4)):
            assert np.array_equal(on[f][solved], per[solved, col]), (k, f)
        assert np.array_equal(on["schedule_digest"][solved], digest[solved]), k
