"""Cases of the expansion's two short cuts in ll_compact.h compactSearch (tests/test_expansion_emu_cpu.py on the CPU emulator,
tests/test_expansion_gpu.py on the device).  HIP-free: the oracle alone.  A case is one A*-epsilon search (w = 1.3) on a map of
at most 32 x 32 cells with the oracle's answer, in the form of tests/row_wait_cases.py, whose cases are part of the set.

The erase at the root: when the popped focal node is the open list's top too, the search neither scans the open array for its
position nor bubbles anything.  The grid of focal counts: a focal path table of at most sixteen columns is looked at by the wave
as four rows of sixteen lanes, one row per successor Wait, Left, Right, Up, with ballots of its own for Down; wider tables keep
the loop over the successors.

  * row_wait_cases: n2, n10, n16, clamp, constraints have sixteen columns (at n16 column 15 holds a real, conflicting agent);
    n32, n64, n66, n80, n128 take the loop.
  * five_a0, five_a8: sixteen agents on an open map.  The searched agent (0 / 8) starts on (10, 10) for (14, 14); at t = 1 one
    agent steps onto each of its five successor cells — onto Right two of them, a count of 2 — and the one that steps onto the
    Wait cell comes from the Up cell: it swaps places with the searched agent's move Up.  Every successor of the first expansion
    is within the focal bound (f = 8, 8, 9, 10, 10 against 10.4), so the counts — Wait 1, Left 1, Right 2, Up 2, Down 1 — decide
    which is expanded next.  five_a0: the agent on Down is in column 15; five_a8: it is in column 0 and the swapping one in
    column 15 (the searched agent's own column is empty, so column 0 can hold somebody only when agent 0 is not the one searched).
  * five32_a0, five32_a8: the same agents and sixteen more that stand still far away: 32 columns, the loop — and the same search.
  * open512: a search of the golden ten-agent trees (bench_instances.json agents10_ex30, the 16th low-level call of its ECBS
    tree) whose open list passes 256 and 512 entries: erases at the root that skip three groups, erases at a position from 256
    on that still scan them.  No search of the 100 golden ten-agent trees has those and an erase of the open array's LAST
    element as well (two of their 21 000 erases are of that kind), so that one is a case of its own, erase_last (agents10_ex40,
    the 11th call).
  * corridor: a map of two cells, (0, 0) to (1, 0), with the goal cell taken at t = 1 .. 3 and waiting forbidden at t = 4: four
    expansions with one successor each — the open list holds one node at every pop — and the goal's."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402
import row_wait_cases as rw  # noqa: E402

W = rw.W
CAP = 100000  # expansions of an oracle search: none of these comes near

# the searched agent of the five_* cases and who steps where at t = 1
FIVE_START, FIVE_GOAL = [10, 10], [14, 14]
ONTO_WAIT_SWAP = [[10, 11], [10, 10]]
ONTO_LEFT = [[8, 10], [9, 10]]
ONTO_RIGHT = ([[12, 10], [11, 10]], [[11, 9], [11, 10]])
ONTO_UP = [[10, 12], [10, 11]]
ONTO_DOWN = [[10, 8], [10, 9]]


def _case(name, inst, agent, ctx_paths, vc=(), ec=()):
    want = oracle.ll_search(oracle.ECBS, inst, agent, inst["starts"][agent], inst["goals"][agent], vertex_constraints=vc,
                            edge_constraints=ec, ctx_paths=ctx_paths, w=W, cap_expansions=CAP)
    assert want["success"] and want["rc"] != -1, name
    return dict(name=name, n=len(inst["starts"]), inst=inst, agent=agent, vc=[list(v) for v in vc], ec=[list(e) for e in ec],
                ctx_paths=ctx_paths, want=want)


def _five(name, n, agent):
    where = {15: ONTO_DOWN, 0: None, 3: ONTO_LEFT, 5: ONTO_RIGHT[0], 6: ONTO_RIGHT[1], 12: ONTO_UP, 1: ONTO_WAIT_SWAP}
    if agent != 0:
        where.update({0: ONTO_DOWN, 15: ONTO_WAIT_SWAP, 1: None})
    paths = []
    for a in range(n):
        p = where.get(a)
        paths.append([list(s) for s in p] if p else [[a % 32, 25 + a // 32]])  # (the others stand still far away)
    paths[agent] = []
    starts = [list(p[0]) if p else list(FIVE_START) for p in paths]
    goals = [list(p[-1]) if p else list(FIVE_GOAL) for p in paths]
    return _case(name, dict(dimx=32, dimy=32, obstacles=[], starts=starts, goals=goals), agent, paths)


def _golden(name, instance, call):
    with open(os.path.join(ROOT, "tests", "golden", "bench_instances.json")) as f:
        inst = json.load(f)[instance]
    _, calls = oracle.mapf_record(oracle.ECBS, inst, w=W)
    c = calls[call]
    case = _case(name, inst, c["agent"], c["ctx_paths"], c["vertex_constraints"], c["edge_constraints"])
    assert (case["want"]["expanded"], [s[1:] for s in case["want"]["states"]]) == (c["expanded"], c["states"]), name
    return case


def _corridor():
    inst = dict(dimx=2, dimy=1, obstacles=[], starts=[[0, 0]], goals=[[1, 0]])
    return _case("corridor", inst, 0, [[]], vc=[[1, 1, 0], [2, 1, 0], [3, 1, 0], [4, 0, 0]])


OWN = ("five_a0", "five_a8", "five32_a0", "five32_a8", "open512", "erase_last", "corridor")
NAMES = rw.NAMES + OWN
GRID = ("n2", "n10", "n16", "clamp", "constraints", "five_a0", "five_a8", "open512", "erase_last")  # sixteen columns
LOOP = ("n32", "n64", "n66", "n80", "n128", "five32_a0", "five32_a8")                              # more
_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = list(rw.cases())
        _CASES += [_five("five_a0", 16, 0), _five("five_a8", 16, 8), _five("five32_a0", 32, 0), _five("five32_a8", 32, 8)]
        _CASES.append(_golden("open512", "map_32by32_obst204_agents10_ex30", 15))
        _CASES.append(_golden("erase_last", "map_32by32_obst204_agents10_ex40", 10))
        _CASES.append(_corridor())
        assert tuple(c["name"] for c in _CASES) == NAMES
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


def expected(c):
    return rw.expected(c)
