"""The LDS tier of MRP_LL_ASTAR_EPS_TA (csrc/ll_compact_ta_eps.h ct::compactSearchTaEps — the kernels' own source) on the CPU
emulator of the wave vocabulary (tests/support/emu_ta_eps.cpp), against the checker (tests/support/ecbs_ta_check.cpp):

  * the corpus of tests/ecbs_ta_corpus.py: a search that finishes in the tier equals the checker bit for bit — status, cost,
    fmin, expansion count, states, and the actions and action costs the engine derives from the states —, every other one
    returns a capacity code or is not tried, and no search touches a byte outside its window; enough searches finish there,
    decrease-key searches among them (w = 2.0 too), and a node sitting in the focal list is re-keyed in place;
  * every limit of the tier from both sides: the node cap (exact, from the checker's node count in front of the last
    expansion), the last state at time 62 / 63, 64 / 65 vertex and edge keys, a 32- / 33-cell side, focalH 511 / 512, and
    a start whose h does not fit f's field.
A search that leaves the tier is run again by the arena tier on the device; here it only has to say so."""
import pytest

import ecbs_ta_checker as checker
import ecbs_ta_corpus
import eps_ta_tier_emu as emu


@pytest.fixture(scope="module")
def replayed(bench_instances):
    cases, _ = ecbs_ta_corpus.generate(checker, bench_instances)
    assert len(cases) == 735
    return [(c, emu.run_case(c)) for c in cases]


def _same(r, o, goal, tag):
    """The tier's answer r against the checker's o."""
    if o["rc"] == -1:
        assert r["status"] == emu.C_CAP_EXP, tag
        return
    assert r["expanded"] == o["expanded"], (tag, r["expanded"], o["expanded"])
    if not o["success"]:
        assert r["status"] == emu.C_NO_SOLUTION, tag
        return
    assert r["status"] == emu.C_OK, tag
    assert (r["cost"], r["fmin"], r["states"]) == (o["cost"], o["fmin"], o["states"]), tag
    assert emu.actions_of(r["states"], goal) == (o["actions"], o["action_costs"]), tag


def test_the_corpus_against_the_checker(replayed):
    finished, dk_finished, dk_w2, rekeys = 0, 0, 0, 0
    for i, (c, r) in enumerate(replayed):
        tag = (i, c["start"], c["goal"], c["w"], len(c["vc"]), len(c["ec"]), r["status"])
        assert r["oob"] == 0, tag
        if not emu.in_tier(r):
            assert r["status"] in emu.CAPACITY + (emu.NOT_TRIED,), tag
            continue
        finished += 1
        _same(r, c["oracle"], c["goal"], tag)
        assert r["decrease_keys"] == c["oracle"]["decrease_keys"], tag
        if r["decrease_keys"]:
            dk_finished += 1
            dk_w2 += 1 if c["w"] == 2.0 else 0
        rekeys += r["focal_rekeys"]
    # what keeps the comparison from passing vacuously
    assert finished >= 300, finished
    assert dk_finished >= 8 and dk_w2 >= 1, (dk_finished, dk_w2)
    assert rekeys >= 1, rekeys


def test_what_is_not_tried_is_what_the_job_itself_rules_out(replayed):
    """More than 64 vertex or edge keys, a map beyond 32 x 32, more than 128 context agents — and nothing else."""
    n = 0
    for c, r in replayed:
        m = c["map"]
        vc_in = [v for v in c["vc"] if 0 <= v[0] < 1024 and 0 <= v[1] < m["dimx"] and 0 <= v[2] < m["dimy"]]
        ec_in = [e for e in c["ec"] if 0 <= e[0] < 1024 and 0 <= e[1] < m["dimx"] and 0 <= e[2] < m["dimy"] and
                 abs(e[3] - e[1]) + abs(e[4] - e[2]) <= 1]
        has_ctx = any(p for a, p in enumerate(c["ctx"]) if a != c["agent"])
        out = (m["dimx"] > 32 or m["dimy"] > 32 or len(vc_in) > 64 or len(ec_in) > 64 or
               (has_ctx and ((len(c["ctx"]) + 15) & ~15) > 128))
        assert (r["status"] == emu.NOT_TRIED) == out, (c["start"], c["goal"], len(vc_in), len(ec_in), len(c["ctx"]))
        n += out
    assert n >= 20  # (the rounds with many constraints, the 136-agent context, the 48 x 48 map)


OPEN8 = dict(dimx=8, dimy=8, obstacles=[[3, 3], [4, 3]])


def _pair(m, start, goal, **kw):
    limits = {k: kw.pop(k) for k in ("open_cap", "max_t", "node_cap") if k in kw}
    o = checker.ll_search(m, start, goal, kw.get("vc", ()), kw.get("ec", ()), w=kw.get("w", 1.3), agent_idx=kw.get("agent", 0),
                          ctx_paths=kw.get("ctx", ()))
    r = emu.search(m, start, goal, kw.get("vc", ()), kw.get("ec", ()), w=kw.get("w", 1.3), agent_idx=kw.get("agent", 0),
                   ctx_paths=kw.get("ctx", ()), **limits)
    assert r["oob"] == 0
    return o, r


def _stays(m, start, goal, **kw):
    o, r = _pair(m, start, goal, **kw)
    assert o["rc"] == 0
    _same(r, o, goal, (start, goal, kw.get("w", 1.3)))
    return o, r


def test_node_cap_exact():
    """Room for five more nodes is asked in front of every expansion.  The checker, capped one expansion short of the last
    real one, says how many nodes there are in front of it (M; earlier expansions have fewer): cap M + 5 stays, M + 4 leaves."""
    start, goal = [1, 1], [6, 6]
    o = checker.ll_search(OPEN8, start, goal, w=1.3)
    assert o["success"] and o["expanded"] >= 3
    before_last = checker.ll_search(OPEN8, start, goal, w=1.3, cap_expansions=o["expanded"] - 2)
    assert before_last["rc"] == -1
    m_nodes = before_last["nodes"]
    assert m_nodes < o["nodes"]
    _stays(OPEN8, start, goal, w=1.3, node_cap=m_nodes + 5)
    _, r = _pair(OPEN8, start, goal, w=1.3, node_cap=m_nodes + 4)
    assert r["status"] == emu.C_CAP_NODES and r["expanded"] == o["expanded"] - 2  # the expansion it left in front of is not counted


def test_open_and_focal_room():
    start, goal = [1, 1], [6, 6]
    o = checker.ll_search(OPEN8, start, goal, w=1.3)
    _stays(OPEN8, start, goal, w=1.3, open_cap=o["nodes"] + 5)  # (an open list never holds more than there are nodes)
    _, r = _pair(OPEN8, start, goal, w=1.3, open_cap=6)         # room for five more: only while the list holds one entry
    assert r["status"] == emu.C_CAP_NODES and r["expanded"] == 1


@pytest.mark.parametrize("w", [1.0, 1.3])
def test_last_state_at_time_62_stays_63_leaves(w):
    """A constraint on the goal cell at time T keeps the agent, which starts there, busy until T + 1: the path's last state
    is at T + 1.  Nodes up to t = 61 are expanded in the tier, so a goal pop at t = 62 is the last one it can make."""
    o, r = _stays(OPEN8, [6, 6], [6, 6], vc=[[61, 6, 6]], w=w)
    assert o["states"][-1][0] == 62 and o["max_time"] == 62
    o, r = _pair(OPEN8, [6, 6], [6, 6], vc=[[62, 6, 6]], w=w)
    assert o["states"][-1][0] == 63
    assert r["status"] == emu.C_CAP_HORIZON
    o, r = _pair(OPEN8, [6, 6], [6, 6], vc=[[20, 6, 6]], w=w, max_t=20)  # the launch's own limit (lds_rows - 2)
    assert o["states"][-1][0] == 21 and r["status"] == emu.C_OK
    _, r = _pair(OPEN8, [6, 6], [6, 6], vc=[[20, 6, 6]], w=w, max_t=19)
    assert r["status"] == emu.C_CAP_HORIZON


def test_64_keys_are_tried_65_are_not():
    far_vc = [[200 + k, k % 6, k // 6 % 6] for k in range(65)]        # (inside the map and the horizon, never the goal cell)
    far_ec = [[200 + k, 0, 0, 1, 0] for k in range(65)]
    near_vc, near_ec = [[2, 2, 1], [3, 2, 2]], [[0, 1, 1, 2, 1]]
    _stays(OPEN8, [1, 1], [6, 6], vc=near_vc + far_vc[:62], ec=near_ec + far_ec[:63])
    _, r = _pair(OPEN8, [1, 1], [6, 6], vc=near_vc + far_vc[:63], ec=near_ec)
    assert r["status"] == emu.NOT_TRIED
    _, r = _pair(OPEN8, [1, 1], [6, 6], vc=near_vc, ec=near_ec + far_ec[:64])
    assert r["status"] == emu.NOT_TRIED
    # a key outside the map or the horizon is dropped by the packer and does not count
    _stays(OPEN8, [1, 1], [6, 6], vc=near_vc + far_vc[:62] + [[5, 8, 0], [1024, 0, 0]], ec=near_ec + far_ec[:63] + [[1, 0, 0, 2, 0]])


def test_32_cells_a_side_are_tried_33_are_not():
    for dimx, dimy, tried in ((32, 6, True), (6, 32, True), (33, 6, False), (6, 33, False)):
        m = dict(dimx=dimx, dimy=dimy, obstacles=[[2, 2], [2, 3]])
        goal = [dimx - 1, dimy - 1]
        if tried:
            _stays(m, [0, 0], goal)
        else:
            _, r = _pair(m, [0, 0], goal)
            assert r["status"] == emu.NOT_TRIED


def _escorted(n_agents, steps):
    """A one-row corridor at w = 1.0 — the focal list holds the straight walk alone — with n_agents others on the very cell
    the agent steps on, at every step: focalH = steps * n_agents at the goal."""
    m = dict(dimx=32, dimy=1, obstacles=[])
    ctx = [[]] + [[[t, 0] for t in range(steps + 1)] for _ in range(n_agents)]
    return _pair(m, [0, 0], [steps, 0], w=1.0, agent=0, ctx=ctx)


def test_focal_heuristic_511_fits_512_does_not():
    o, r = _escorted(73, 7)
    assert o["success"] and o["cost"] == 7
    _same(r, o, [7, 0], "focalH 511")
    o, r = _escorted(64, 8)
    assert o["success"] and o["cost"] == 8
    assert r["status"] == emu.C_OVERFLOW


def _serpentine():
    """32 x 32, walls on the odd rows with a gap at alternating ends: (0, 0) is 4 * 31 + 8 = 132 steps from (0, 8)."""
    obst = []
    for y in range(1, 9, 2):
        gap = 31 if y % 4 == 1 else 0
        obst += [[x, y] for x in range(32) if x != gap]
    return dict(dimx=32, dimy=32, obstacles=obst)


def test_a_start_whose_h_does_not_fit_leaves_at_once():
    m = _serpentine()
    assert ecbs_ta_corpus.bfs_table(32, 32, m["obstacles"], [0, 8])[0][0] == 132
    r = emu.search(m, [0, 0], [0, 8], w=1.3)
    assert r["status"] == emu.C_CAP_HORIZON and r["expanded"] == 0 and r["oob"] == 0
    # ... and 124 is the last h that fits: from (8, 0), 132 - 8 steps out, the search runs until its f outgrows the field
    assert ecbs_ta_corpus.bfs_table(32, 32, m["obstacles"], [0, 8])[0][8] == 124
    r = emu.search(m, [8, 0], [0, 8], w=1.3)
    assert r["status"] in emu.CAPACITY and r["expanded"] >= 1 and r["oob"] == 0
