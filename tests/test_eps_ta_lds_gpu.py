"""MRP_LL_JOB_TRY_LDS on the MI355X: MRP_LL_ASTAR_EPS_TA searches that start in their LDS tier (csrc/ll_compact_ta_eps.h
through ll_ta.h runTaEpsLds) and go on in the arena tier when they outgrow it.

The yardsticks: the CPU checker (tests/support/ecbs_ta_check.cpp) for every answer — status, cost, fmin, expansion count,
states, actions, action costs, flagged or not —, and the emulator's run of the same tier (tests/eps_ta_tier_emu.py) for
WHERE a search ends: tier == 0 exactly for the searches the emulator finished in the tier, tier == 1 for the rest.  The flag
is a hint: the unflagged twin of every job gives the same fields with tier == 1."""
import os

import pytest

import ecbs_ta_checker as checker
import ecbs_ta_corpus
import ecbs_ta_tree_corpus as tree_corpus
import eps_ta_tier_emu as emu

pytestmark = pytest.mark.gpu


def _but_tier(r):
    return (r.status, r.success, r.cost, r.fmin, r.expanded, r.n_states, r.states, r.actions, r.action_costs)


def _same_as_checker(r, o, tag):
    from libmultirobotplanning_amd import ll
    assert r.status not in (ll.CAP_NODES, ll.CAP_HORIZON, ll.CAP_FOCAL, ll.BAD_JOB), tag
    if o["rc"] == -1:
        assert r.status == ll.CAP_EXPANSIONS, tag
        return
    assert (r.success, r.expanded) == (o["success"], o["expanded"]), (tag, r.status, r.expanded, o["expanded"])
    if o["success"]:
        assert r.status == ll.OK, tag
        assert (r.cost, r.fmin, r.states, r.actions, r.action_costs) == (o["cost"], o["fmin"], o["states"], o["actions"],
                                                                         o["action_costs"]), tag
    else:
        assert r.status == ll.NO_SOLUTION, tag


class _Bench:
    """One engine; maps and heuristic tables by content, uploaded before any session begins."""

    def __init__(self, slots=64, store=0):
        from libmultirobotplanning_amd import ll
        self.ll = ll
        self.eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=slots)
        if store:
            self.eng.path_store_reserve(store)
        self.maps, self.heurs = {}, {}

    def close(self):
        self.eng.close()

    def map_id(self, m):
        key = (m["dimx"], m["dimy"], tuple(map(tuple, m["obstacles"])))
        if key not in self.maps:
            self.maps[key] = self.eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        return self.maps[key]

    def heur_id(self, m, g):
        key = (self.map_id(m), tuple(g))
        if key not in self.heurs:
            self.heurs[key] = self.eng.upload_heuristic(key[0], ecbs_ta_corpus.bfs_table(m["dimx"], m["dimy"], m["obstacles"], g))
        return self.heurs[key]

    def job(self, c, try_lds, ids=None, out=-1):
        g = c["goal"]
        return self.ll.LLJob(map_id=self.map_id(c["map"]), algo=self.ll.ASTAR_EPS_TA, start=c["start"], goal=g,
                             agent_idx=c["agent"], w=c["w"], vertex_constraints=c["vc"], edge_constraints=c["ec"],
                             ctx_paths=c["ctx"], max_expansions=c["cap"], heuristic_id=-1 if g is None else self.heur_id(c["map"], g),
                             try_lds=try_lds, path_ids=ids, result_path_id=out)


def _case(m, start, goal, w=1.3, vc=(), ec=(), agent=0, ctx=(), cap=-1):
    o = checker.ll_search(m, start, goal, vc, ec, w=w, agent_idx=agent, ctx_paths=ctx, cap_expansions=cap)
    return dict(map=m, start=start, goal=goal, vc=list(vc), ec=list(ec), w=w, agent=agent, ctx=[list(p) for p in ctx], cap=cap, oracle=o)


@pytest.fixture(scope="module")
def corpus(bench_instances):
    """The corpus and, case by case, whether the emulator's run of the tier finished there."""
    cases, _ = ecbs_ta_corpus.generate(checker, bench_instances)
    stays = [emu.in_tier(emu.run_case(c)) for c in cases]
    assert sum(stays) >= 300 and len(cases) - sum(stays) >= 200
    assert sum(1 for c, s in zip(cases, stays) if s and c["oracle"]["decrease_keys"] > 0) >= 8
    return cases, stays


def _flagged_and_not(b, cases, stays, where):
    flagged = b.eng.search_batch([b.job(c, True) for c in cases])
    plain = b.eng.search_batch([b.job(c, False) for c in cases])
    assert len(flagged) == len(plain) == len(cases)
    for i, (c, s, f, p) in enumerate(zip(cases, stays, flagged, plain)):
        tag = (where, i, c["start"], c["goal"], c["w"], len(c["vc"]), len(c["ec"]), f.status, f.tier)
        _same_as_checker(f, c["oracle"], tag)
        assert f.tier == (0 if s else 1), tag   # without the tier every search reports tier 1: this is where the test fails
        assert p.tier == 1, tag
        assert _but_tier(f) == _but_tier(p), tag


def test_corpus_flagged_in_a_batch_and_in_a_mixed_session(corpus):
    cases, stays = corpus
    b = _Bench(slots=256)
    try:
        _flagged_and_not(b, cases, stays, "batch")
        b.eng.session_begin(64)
        try:
            _flagged_and_not(b, cases[:100], stays[:100], "session")
        finally:
            b.eng.session_end()
    finally:
        b.close()


OPEN32 = dict(dimx=32, dimy=32, obstacles=[])


def test_by_slot_and_stored_result_flagged():
    """Two searches leave their paths in store slots; a third names them by slot, flagged, and stores its own; a fourth reads
    all three.  Same answers as the checker's and as the shipped, unflagged twins'; the flagged ones end in the tier."""
    b = _Bench(slots=16, store=16)
    try:
        first = [_case(OPEN32, [4, 14], [14, 14]), _case(OPEN32, [14, 8], [14, 20], w=2.0)]
        res = b.eng.search_batch([b.job(c, True, out=k) for k, c in enumerate(first)])
        for k, (c, r) in enumerate(zip(first, res)):
            _same_as_checker(r, c["oracle"], ("stored", k))
            assert r.tier == 0
        paths = [[s[1:] for s in r.states] for r in res]
        third = _case(OPEN32, [20, 14], [6, 14], agent=2, ctx=[paths[0], paths[1], []])
        assert emu.in_tier(emu.run_case(third))
        by_slot, shipped = b.eng.search_batch([b.job(third, True, ids=[0, 1, -1], out=2), b.job(third, False)])
        _same_as_checker(by_slot, third["oracle"], "by slot")
        assert by_slot.tier == 0 and shipped.tier == 1 and _but_tier(by_slot) == _but_tier(shipped)
        paths.append([s[1:] for s in by_slot.states])
        fourth = _case(OPEN32, [14, 22], [14, 6], agent=3, ctx=paths + [[]], w=2.0)
        assert emu.in_tier(emu.run_case(fourth))
        got = b.eng.search_batch([b.job(fourth, True, ids=[0, 1, 2, -1])])[0]
        _same_as_checker(got, fourth["oracle"], "reads the flagged search's slot")
        assert got.tier == 0
        alone = checker.ll_search(OPEN32, [14, 22], [14, 6], w=2.0)
        assert (alone["expanded"], alone["states"]) != (got.expanded, got.states)  # the contexts are seen
    finally:
        b.close()


def _serpentine():
    """32 x 32, walls on the odd rows with a gap at alternating ends: (0, 0) is 132 steps from (0, 8), beyond f's field."""
    obst = []
    for y in range(1, 9, 2):
        gap = 31 if y % 4 == 1 else 0
        obst += [[x, y] for x in range(32) if x != gap]
    return dict(dimx=32, dimy=32, obstacles=obst)


def _escort(n_agents, steps):
    m = dict(dimx=32, dimy=1, obstacles=[])
    ctx = [[]] + [[[t, 0] for t in range(steps + 1)] for _ in range(n_agents)]
    return _case(m, [0, 0], [steps, 0], w=1.0, agent=0, ctx=ctx)


def test_the_limits_hand_over_and_the_answer_is_the_checkers():
    """Each limit of the tier from both sides (the emulator says which side): the last state at time 62 / 63, 64 / 65 vertex
    and edge keys, a 32- / 33-cell side, a focalH that fits / overflows, a start whose h does not fit."""
    open8 = dict(dimx=8, dimy=8, obstacles=[[3, 3], [4, 3]])
    far_vc = [[200 + k, k % 6, k // 6 % 6] for k in range(65)]
    far_ec = [[200 + k, 0, 0, 1, 0] for k in range(65)]
    cases = [_case(open8, [6, 6], [6, 6], vc=[[61, 6, 6]]), _case(open8, [6, 6], [6, 6], vc=[[62, 6, 6]]),
             _case(open8, [1, 1], [6, 6], vc=far_vc[:64], ec=far_ec[:64]), _case(open8, [1, 1], [6, 6], vc=far_vc[:65]),
             _case(open8, [1, 1], [6, 6], ec=far_ec[:65]),
             _case(dict(dimx=32, dimy=6, obstacles=[[2, 2]]), [0, 0], [31, 5]), _case(dict(dimx=33, dimy=6, obstacles=[[2, 2]]), [0, 0], [32, 5]),
             _escort(73, 7), _escort(64, 8), _case(_serpentine(), [0, 0], [0, 8])]
    stays = [emu.in_tier(emu.run_case(c)) for c in cases]
    assert stays == [True, False, True, False, False, True, False, True, False, False]
    b = _Bench()
    try:
        _flagged_and_not(b, cases, stays, "limits")
    finally:
        b.close()


@pytest.mark.parametrize("tiers", [dict(lds_nodes=-1), dict(lds_path_bytes=1024)])
def test_the_flag_is_harmless_without_the_tier(corpus, tiers):
    """The LDS tier off, or its path area too small for the tier's two tables: flagged jobs run in the arena tier."""
    cases, stays = corpus
    pick = [k for k, s in enumerate(stays) if s][:12] + [k for k, s in enumerate(stays) if not s][:4]
    b = _Bench()
    try:
        b.eng.configure_tiers(**tiers)
        res = b.eng.search_batch([b.job(cases[k], True) for k in pick])
        for k, r in zip(pick, res):
            _same_as_checker(r, cases[k]["oracle"], (tiers, k))
            assert r.tier == 1, (tiers, k)
    finally:
        b.close()


def test_the_driver_knob_changes_no_solution(ref_tests, oracle_mod, monkeypatch):
    """hl.solve_ecbs_ta_batch at w = 1.3 with MRP_HL_TA_EPS_LDS set and unset, roots as dependent jobs (every search a job) and
    as one call, and with the device path store: identical solutions, equal to the sequential restatement."""
    from libmultirobotplanning_amd import hl
    insts = tree_corpus.corpus()[:6] + list(tree_corpus.ref_inputs(ref_tests).values())
    w = 1.3
    assert "MRP_HL_TA_EPS_LDS" not in os.environ
    for use_root_kernel, device_paths in ((False, False), (True, False), (False, True)):
        if device_paths:
            monkeypatch.setenv("MRP_HL_TA_DEVICE_PATHS", "1")
        monkeypatch.delenv("MRP_HL_TA_EPS_LDS", raising=False)
        off, _ = hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=use_root_kernel)
        monkeypatch.setenv("MRP_HL_TA_EPS_LDS", "1")
        on, _ = hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=use_root_kernel)
        assert on == off, (use_root_kernel, device_paths)
        for g, i in zip(on, insts):
            tree_corpus.same(g, tree_corpus.reference(i, w))
