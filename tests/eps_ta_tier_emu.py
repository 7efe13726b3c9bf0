"""ctypes loader of tests/support/emu_ta_eps.cpp: ONE search of the LDS tier of MRP_LL_ASTAR_EPS_TA (ct::compactSearchTaEps,
csrc/ll_compact_ta_eps.h — the kernels' own source) on the CPU emulator of the wave vocabulary, built into tests/_build/ on
first use.  Shared by the emulator test and by the GPU test, which asks it which cases finish in the tier."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P, I64P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
C_OK, C_NO_SOLUTION, C_CAP_EXP, C_CAP_NODES, C_CAP_HORIZON, C_BAD, C_OVERFLOW, NOT_TRIED = 0, 1, 2, 3, 4, 5, -1, 100
CAPACITY = (C_CAP_NODES, C_CAP_HORIZON, C_OVERFLOW)  # the search leaves the tier: the arena tier runs it from the start
OPEN_CAP, MAX_T, NODE_CAP = 1023, 61, 1023           # the tier's own limits (csrc/ll_compact_ta_eps.h)
ACT_UP, ACT_DOWN, ACT_LEFT, ACT_RIGHT, ACT_WAIT = 0, 1, 2, 3, 4  # include/mrp_ll.h MRP_LL_ACT_*
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, "libemu_ta_eps.so")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [os.path.join(ROOT, "tests", "support", "emu_ta_eps.cpp"), os.path.join(ROOT, "tests", "support", "wave_emu.h"),
            os.path.join(csrc, "ll_compact_ta_eps.h"), os.path.join(csrc, "ll_compact.h"), os.path.join(csrc, "host", "ll_pack.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, deps[0]])
        os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.emu_ta_eps_search.restype = ctypes.c_int
    L.emu_ta_eps_search.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, I32P, ctypes.c_float,
                                    ctypes.c_int, ctypes.c_int, I32P, I32P, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, I64P, I32P, ctypes.c_int]
    _lib = L
    return L


def _i32(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(shape))
    return a, a.ctypes.data_as(I32P)


def search(inst_map, start, goal, vertex_constraints=(), edge_constraints=(), w=1.0, agent_idx=0, ctx_paths=(),
           cap_expansions=-1, open_cap=OPEN_CAP, max_t=MAX_T, node_cap=NODE_CAP, horizon=1024):
    """One search, arguments as ecbs_ta_checker.ll_search.  Returns status (C_*; NOT_TRIED: the job itself does not fit the
    tier), cost, fmin, expanded, nodes, states [t, x, y], oob (out-of-window LDS reads + writes), decrease_keys,
    focal_rekeys (decrease-key events on a node sitting in the focal list)."""
    obst, obst_p = _i32(inst_map["obstacles"], (-1, 2))
    vc, vc_p = _i32(vertex_constraints, (-1, 3))
    ec, ec_p = _i32(edge_constraints, (-1, 5))
    plen, plen_p = _i32([len(p) for p in ctx_paths], (-1,))
    pxy, pxy_p = _i32([xy for p in ctx_paths for xy in p], (-1, 2))
    out = np.zeros(10, dtype=np.int64)
    cells = np.zeros(64, dtype=np.int32)
    g = goal if goal is not None else (0, 0)
    rc = lib().emu_ta_eps_search(inst_map["dimx"], inst_map["dimy"], len(obst), obst_p, start[0], start[1],
                                 0 if goal is None else 1, g[0], g[1], len(vc), vc_p, len(ec), ec_p, w, agent_idx, len(plen),
                                 plen_p, pxy_p, cap_expansions, horizon, open_cap, max_t, node_cap, out.ctypes.data_as(I64P),
                                 cells.ctypes.data_as(I32P), len(cells))
    assert rc >= -1, rc
    if rc == NOT_TRIED:
        return dict(status=NOT_TRIED, oob=0, decrease_keys=0, focal_rekeys=0, expanded=0, nodes=0)
    assert rc == out[0]
    n = int(out[3]) if rc == C_OK else 0
    return dict(status=rc, cost=int(out[1]), fmin=int(out[2]), expanded=int(out[4]), nodes=int(out[5]),
                states=[[k, int(cells[k]) & 0xFF, int(cells[k]) >> 8] for k in range(n)], oob=int(out[6] + out[7]),
                decrease_keys=int(out[8]), focal_rekeys=int(out[9]))


def run_case(c, **limits):
    return search(c["map"], c["start"], c["goal"], c["vc"], c["ec"], w=c["w"], agent_idx=c["agent"], ctx_paths=c["ctx"],
                  cap_expansions=c["cap"], **limits)


def actions_of(states, goal):
    """Actions and action costs from the states, as the engine derives them (csrc/host/ll_unpack.h): a Wait at the goal —
    anywhere for an agent without a task — is free."""
    acts, costs = [], []
    for (_, x0, y0), (_, x1, y1) in zip(states, states[1:]):
        d = (x1 - x0, y1 - y0)
        acts.append({(0, 0): ACT_WAIT, (-1, 0): ACT_LEFT, (1, 0): ACT_RIGHT, (0, 1): ACT_UP, (0, -1): ACT_DOWN}[d])
        at_goal = goal is None or [x0, y0] == list(goal)
        costs.append(0 if d == (0, 0) and at_goal else 1)
    return acts, costs


def in_tier(r):
    """The search gave its answer inside the tier (what the device reports as tier == 0)."""
    return r["status"] in (C_OK, C_NO_SOLUTION, C_CAP_EXP, C_BAD)
