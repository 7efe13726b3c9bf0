"""Cases of the focal-table row loads' lane mask (tests/test_row_wait_emu_cpu.py on the CPU emulator,
tests/test_row_wait_gpu.py on the device).  HIP-free: the oracle alone.

The searches that read the focal path table from device memory (ll_compact.h compactSearch, PLDS = false) load one table
column per lane.  A lane beyond the row's end is clamped to the row's LAST column — every read stays inside the table — and
what it has loaded must not be counted: the loads are unmasked, the lanes are left out where the values are counted.  A
search shows a missing mask only where

  * the table has clamped lanes at all: its width (the agent count rounded up to 16) is no multiple of 64, and
  * its last column holds a real agent: the agent count is a multiple of 16, and
  * that agent's path touches the searched agent's successors (a clamped lane counts it a second time, 48 lanes 48 times).

A case is one search of agent 0 (never the last agent) of an n-agent instance on a 32 x 32 map, against the paths of all
others.  Rows 0 and 4 are walls, and so is row 2 from x = 3 to x = 8: agent 0, from (2, 2) to (9, 2), has two ways of nine
steps, along row 1 and along row 3, and nothing shorter than 13 around them (w = 1.3: 11.7).  The LAST agent comes along row 1
the other way, from (9, 1) to (2, 1): it stands on a successor's cell at t + 1 and swaps places with agent 0 where they meet —
one conflict on the upper way.  The two agents in front of it (where the instance has four or more) stand in row 3, on
(5, 3) and (7, 3): two conflicts on the lower way.  So the search takes the upper way — unless the last agent is counted more
than once.  Agent 1 (from five agents on) walks twelve steps along row 20, so that the table has more rows than the search
has time steps; every other agent stands still in rows 10 to 13.
The counts 2, 10, 64, 66 and 128 give tables of 16, 16, 64, 80 and 128 columns whose last column is empty (or, at 64 and 128,
that have no clamped lane): they pin the counting itself (at 66, columns 64 and 65 hold conflicting agents).  16, 32 and 80
agents (80: the second row load's clamped lanes) have a real agent in the last column below clamped lanes: the cases a missing
mask fails.  `clamp` is the 16-agent case without agent 1's walk and with a last agent that only steps from (6, 1) to (5, 1):
a table of two rows, every expansion from t = 1 on reads row tPad - 1 twice.  `constraints` is the 16-agent case with a vertex
constraint on the upper way, one on the lower way and an edge constraint on agent 0's first step down."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402

W = 1.3
CAP = 3000  # expansions of an oracle search: none of these comes near
START, GOAL = [2, 2], [9, 2]
OBSTACLES = [[x, 0] for x in range(32)] + [[x, 4] for x in range(32)] + [[x, 2] for x in range(3, 9)]


def _instance(n, short):
    starts = [list(START)] + [[i % 32, 10 + i // 32] for i in range(1, n)]
    goals = [list(GOAL)] + [list(s) for s in starts[1:]]
    starts[n - 1], goals[n - 1] = ([6, 1], [5, 1]) if short else ([9, 1], [2, 1])
    if n >= 4:
        starts[n - 3] = goals[n - 3] = [5, 3]
        starts[n - 2] = goals[n - 2] = [7, 3]
    if n >= 5 and not short:
        starts[1], goals[1] = [0, 20], [12, 20]
    return dict(dimx=32, dimy=32, obstacles=[list(o) for o in OBSTACLES], starts=starts, goals=goals)


def _alone(inst, a):
    o = oracle.ll_search(oracle.ECBS, inst, a, inst["starts"][a], inst["goals"][a], ctx_paths=[[] for _ in inst["starts"]], w=W,
                         cap_expansions=CAP)
    assert o["success"]
    return [s[1:] for s in o["states"]]


def make_case(name, n, vc=(), ec=(), short=False):
    """dict(name, n, inst, agent, vc, ec, ctx_paths (agent 0's own: []), want = the oracle's search, sensitive)."""
    inst = _instance(n, short)
    paths = [[]] + [_alone(inst, a) for a in range(1, n)]
    want = oracle.ll_search(oracle.ECBS, inst, 0, inst["starts"][0], inst["goals"][0], vertex_constraints=vc, edge_constraints=ec,
                            ctx_paths=paths, w=W, cap_expansions=CAP)
    assert want["success"] and want["rc"] != -1
    return dict(name=name, n=n, inst=inst, agent=0, vc=[list(v) for v in vc], ec=[list(e) for e in ec], ctx_paths=paths, want=want,
                sensitive=n % 16 == 0 and n % 64 != 0)


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = [make_case("n%d" % n, n) for n in (2, 10, 64, 66, 128, 16, 32, 80)]
        _CASES.append(make_case("clamp", 16, short=True))
        _CASES.append(make_case("constraints", 16, vc=[[4, 5, 1], [6, 6, 3]], ec=[[0, 2, 2, 2, 3]]))
    return _CASES


NAMES = ("n2", "n10", "n64", "n66", "n128", "n16", "n32", "n80", "clamp", "constraints")


def case(name):
    return next(c for c in cases() if c["name"] == name)


def expected(c):
    w = c["want"]
    return dict(status=0, cost=w["cost"], fmin=w["fmin"], n_states=len(w["states"]), expanded=w["expanded"], states=w["states"])
