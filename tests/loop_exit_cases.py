"""Cases of the search loop's top and exits in ll_compact.h compactSearch (tests/test_select_stores_emu_cpu.py on the CPU
emulator, tests/test_select_stores_gpu.py on the device).  HIP-free: the oracle alone.  A case is one A*-epsilon search
(w = 1.3) on a map of at most 8 x 8 cells, in the form of tests/expansion_cases.py, with the knobs of the tier it runs under:

  max_exp    expansion cap (-1: none)          open_cap, max_t   tighter limits of the tier (0: the tier's own)
  kind       "oracle": the search ends inside the tier, every output word is the oracle's
             "cap":    the cap is one below the search's expansions: status 2, expanded = the cap + 1 (the pop that passed
                       the cap is counted, a_star_epsilon.hpp:193)
             "overflow": the search leaves the tier: status -1, `code` in cost (1 open entries, 2 t > maxT, 3 focalH field),
                       `expanded` pops before it
  forms      the forms of the tier the case is for (an overflow of the narrow focalH field is none of the wide one's)

The cases:
  * start_is_goal: the start node is the goal pop.
  * walled_in: one cell, start = goal, the cell taken at t = 1 and 2: no successor, the open list runs empty.
  * goal_early: a corridor of four cells with the goal cell taken at t = 5: the agent arrives at t = 3 — the goal cell is
    popped at t <= lastGoal, which is no goal and expands — and must come back.  cap_exact / cap_minus_one: the same search
    with a cap equal to its expansions and one below.
  * over_open, over_t: an open 8 x 8 map, corner to corner, with room for 12 open entries / time steps up to 3.
  * over_fh: a corridor of three cells; 127 agents stand on the middle one, the start is taken from t = 1 on and the goal
    cell at t = 2 .. 4, so the agent has to step into the crowd (focalH 127) and wait there (each of the 127 is on the cell
    at t + 1 and, the cell being the one the agent comes from too, counts as a swap as well: 254 more).  With 128 columns the
    narrow tier hands over at a popped focalH above 255 — the pop at t = 2, focalH 381; the wide entry has six bits of
    focalH: its first expansion's successor does not fit.
  * open_only: a corridor of four cells, from (2, 0) to (0, 0): Wait (f = 3) and Right (f = 4) are outside the focal bound
    (2.6), Left is inside: a turn of two, then a turn with one push into the open list and none into the focal list.
  * wait8: the open 8 x 8 map, corner to corner, with the goal cell taken at t = 20: open and focal lists of a hundred
    entries and more — heaps crossing 31 / 32 and 63 / 64 entries with the other list shorter, second chains one level
    deeper, pops that empty the focal list."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402

W = 1.3
REF_CAP = 200000
ALL_FORMS = ("bitmap_in_lds", "bitmap_in_memory", "wide")
_CASES = None


def _ref(inst, agent, vc, ctx_paths, cap=REF_CAP):
    return oracle.ll_search(oracle.ECBS, inst, agent, inst["starts"][agent], inst["goals"][agent], vertex_constraints=vc,
                            edge_constraints=[], ctx_paths=ctx_paths, w=W, cap_expansions=cap)


def _case(name, inst, vc=(), ctx_paths=None, kind="oracle", max_exp=-1, open_cap=0, max_t=0, code=0, forms=ALL_FORMS):
    ctx_paths = [[] for _ in inst["starts"]] if ctx_paths is None else ctx_paths
    vc = [list(v) for v in vc]
    want = _ref(inst, 0, vc, ctx_paths)
    assert want["rc"] != -1, name
    return dict(name=name, inst=inst, agent=0, vc=vc, ec=[], ctx_paths=ctx_paths, kind=kind, max_exp=max_exp, open_cap=open_cap,
                max_t=max_t, code=code, forms=forms, want=want)


def _corridor(n, start, goal, others=()):
    return dict(dimx=n, dimy=1, obstacles=[], starts=[[start, 0]] + [list(o) for o in others],
                goals=[[goal, 0]] + [list(o) for o in others])


def _open8():
    return dict(dimx=8, dimy=8, obstacles=[], starts=[[0, 0]], goals=[[7, 7]])


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = [_case("start_is_goal", dict(dimx=4, dimy=4, obstacles=[], starts=[[1, 1]], goals=[[1, 1]])),
           _case("walled_in", dict(dimx=1, dimy=1, obstacles=[], starts=[[0, 0]], goals=[[0, 0]]), vc=[[1, 0, 0], [2, 0, 0]])]
    early = _case("goal_early", _corridor(4, 0, 3), vc=[[5, 3, 0]])
    e = early["want"]["expanded"]
    out += [early, _case("cap_exact", _corridor(4, 0, 3), vc=[[5, 3, 0]], max_exp=e),
            _case("cap_minus_one", _corridor(4, 0, 3), vc=[[5, 3, 0]], kind="cap", max_exp=e - 1)]
    out += [_case("over_open", _open8(), kind="overflow", open_cap=12, code=1),
            _case("over_t", _open8(), kind="overflow", max_t=3, code=2)]
    crowd = [[1, 0]] * 127
    inst = _corridor(3, 0, 2, crowd)
    ctx = [[]] + [[list(c)] for c in crowd]
    vc = [[t, 0, 0] for t in range(1, 6)] + [[t, 2, 0] for t in (2, 3, 4)]
    out += [_case("over_fh_narrow", inst, vc=vc, ctx_paths=ctx, kind="overflow", code=3, forms=ALL_FORMS[:2]),
            _case("over_fh_wide", inst, vc=vc, ctx_paths=ctx, kind="overflow", code=3, forms=ALL_FORMS[2:])]
    out += [_case("open_only", _corridor(4, 2, 0)), _case("wait8", _open8(), vc=[[20, 7, 7]])]
    _CASES = out
    return out


NAMES = ("start_is_goal", "walled_in", "goal_early", "cap_exact", "cap_minus_one", "over_open", "over_t", "over_fh_narrow",
         "over_fh_wide", "open_only", "wait8")


def forms_of(name):
    """The forms of the tier a case is for (known without the oracle: the tests parametrise over it)."""
    return {"over_fh_narrow": ALL_FORMS[:2], "over_fh_wide": ALL_FORMS[2:]}.get(name, ALL_FORMS)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def expected(c):
    """The oracle's words of a case of kind "oracle": status (0 found, 1 no path), cost, fmin, n_states, expanded, states."""
    w = c["want"]
    if not w["success"]:
        return dict(status=1, cost=0, fmin=0, n_states=0, expanded=w["expanded"], states=[])
    return dict(status=0, cost=w["cost"], fmin=w["fmin"], n_states=len(w["states"]), expanded=w["expanded"],
                states=[list(s[1:]) for s in w["states"]])


def dump(path):
    """The cases as numbers, for tests/support/select_sanitize_main.cpp: the format of tests/push_cases.py's dump with
    max_exp open_cap max_t, the kind (0 oracle, 1 cap, 2 overflow), its code and a mask of the forms in front of the oracle's
    five words."""
    with open(path, "w") as f:
        for c in cases():
            inst, want = c["inst"], expected(c) if c["want"]["success"] or c["kind"] == "oracle" else None
            flat = lambda rows: [v for r in rows for v in r]  # noqa: E731
            n = [inst["dimx"], inst["dimy"], len(inst["obstacles"])] + flat(inst["obstacles"]) + inst["starts"][0] + inst["goals"][0]
            n += [len(c["vc"])] + flat(c["vc"]) + [0, len(c["ctx_paths"]), 0]
            n += [len(p) for p in c["ctx_paths"]] + flat(flat(c["ctx_paths"]))
            n += [c["max_exp"], c["open_cap"], c["max_t"], ("oracle", "cap", "overflow").index(c["kind"]), c["code"],
                  sum(1 << ALL_FORMS.index(k) for k in c["forms"])]
            n += [want[k] for k in ("status", "cost", "fmin", "n_states", "expanded")]
            f.write(c["name"] + " " + " ".join(str(int(v)) for v in n) + "\n")


if __name__ == "__main__":
    dump(sys.argv[1])
