"""ctypes loader of tests/support/ecbs_ta_check.cpp: the CPU checker of MRP_LL_ASTAR_EPS_TA (AStarEpsilon over the
task-assignment Environment, and ecbs_ta.hpp's conflict tree for one fixed assignment), built from the oracle's headers into
tests/_build/ on first use."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = ctypes.POINTER(ctypes.c_int32)
I64P = ctypes.POINTER(ctypes.c_int64)
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, "libecbs_ta_check.so")
    src = os.path.join(ROOT, "tests", "support", "ecbs_ta_check.cpp")
    deps = [src] + [os.path.join(ROOT, "oracle", h) for h in ("search_restated.hpp", "ta_restated.hpp", "mapf_restated.hpp",
                                                              "heap_restated.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "oracle"),
                               "-o", tmp, src])
        os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.ecbs_ta_ll_search.restype = ctypes.c_int
    L.ecbs_ta_ll_search.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, I32P, ctypes.c_float,
                                    ctypes.c_int, ctypes.c_int, I32P, I32P, ctypes.c_int64, I32P, I64P, I32P, I32P, I32P,
                                    ctypes.c_int]
    L.ecbs_ta_fixed.restype = ctypes.c_int64
    L.ecbs_ta_fixed.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, I32P, I32P, ctypes.c_float,
                                ctypes.c_int64, I64P, I32P, I32P, ctypes.c_int64, I32P]
    _lib = L
    return L


def _i32(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(shape))
    return a, a.ctypes.data_as(I32P)


def ll_search(inst_map, start, goal, vertex_constraints=(), edge_constraints=(), w=1.0, agent_idx=0, ctx_paths=(),
              cap_expansions=-1, cap=1024):
    """One low-level search of ECBS-TA: goal = None for an agent without a task; ctx_paths = the solution vector the search
    sees, per agent [[x, y], ...] ([] = no path yet; agent_idx's own entry is ignored).  Returns rc (-1: expansion cap),
    success, cost, fmin, expanded, states [t, x, y], actions, action_costs, decrease_keys, nodes, max_time."""
    obst, obst_p = _i32(inst_map["obstacles"], (-1, 2))
    vc, vc_p = _i32(vertex_constraints, (-1, 3))
    ec, ec_p = _i32(edge_constraints, (-1, 5))
    plen, plen_p = _i32([len(p) for p in ctx_paths], (-1,))
    pxy, pxy_p = _i32([xy for p in ctx_paths for xy in p], (-1, 2))
    out = np.zeros(8, dtype=np.int32)
    expanded = np.zeros(1, dtype=np.int64)
    states = np.zeros((cap, 3), dtype=np.int32)
    actions = np.zeros(cap, dtype=np.int32)
    costs = np.zeros(cap, dtype=np.int32)
    g = goal if goal is not None else (0, 0)
    rc = lib().ecbs_ta_ll_search(inst_map["dimx"], inst_map["dimy"], len(obst), obst_p, start[0], start[1],
                                 0 if goal is None else 1, g[0], g[1], len(vc), vc_p, len(ec), ec_p, w, agent_idx, len(plen),
                                 plen_p, pxy_p, cap_expansions, out.ctypes.data_as(I32P), expanded.ctypes.data_as(I64P),
                                 states.ctypes.data_as(I32P), actions.ctypes.data_as(I32P), costs.ctypes.data_as(I32P), cap)
    n = int(out[3])
    assert n <= cap
    return dict(rc=rc, success=bool(out[0]), cost=int(out[1]), fmin=int(out[2]), expanded=int(expanded[0]),
                states=states[:n].tolist(), actions=actions[:max(n - 1, 0)].tolist(),
                action_costs=costs[:max(n - 1, 0)].tolist(), decrease_keys=int(out[4]), nodes=int(out[5]),
                max_time=int(out[6]))


def fixed_tree(inst_map, starts, tasks, w, max_high_level=100000):
    """ecbs_ta.hpp's conflict tree for ONE fixed assignment (tasks[i] = [x, y] or None).  Returns (summary, low-level calls);
    a call carries everything the search saw (constraints, ctx_paths) and returned."""
    obst, obst_p = _i32(inst_map["obstacles"], (-1, 2))
    st, st_p = _i32(starts, (-1, 2))
    tk, tk_p = _i32([t if t is not None else [-1, -1] for t in tasks], (-1, 2))
    n = len(starts)
    stats = np.zeros(3, dtype=np.int64)
    end = np.zeros((n, 3), dtype=np.int32)
    ncalls = np.zeros(1, dtype=np.int32)
    words = 1 << 16
    while True:
        buf = np.zeros(words, dtype=np.int32)
        need = lib().ecbs_ta_fixed(inst_map["dimx"], inst_map["dimy"], len(obst), obst_p, n, st_p, tk_p, w, max_high_level,
                                   stats.ctypes.data_as(I64P), end.ctypes.data_as(I32P), buf.ctypes.data_as(I32P), words,
                                   ncalls.ctypes.data_as(I32P))
        if need <= words:
            break
        words = int(need)
    calls = []
    p = 0
    for _ in range(int(ncalls[0])):
        agent, has, tx, ty, ok, cost, fmin, expanded, dk, nvc, nec, nst, nctx = (int(v) for v in buf[p:p + 13])
        p += 13
        vc = buf[p:p + 3 * nvc].reshape(-1, 3).tolist(); p += 3 * nvc
        ec = buf[p:p + 5 * nec].reshape(-1, 5).tolist(); p += 5 * nec
        states = buf[p:p + 3 * nst].reshape(-1, 3).tolist(); p += 3 * nst
        actions = buf[p:p + max(nst - 1, 0)].tolist(); p += max(nst - 1, 0)
        costs = buf[p:p + max(nst - 1, 0)].tolist(); p += max(nst - 1, 0)
        ctx = []
        for _a in range(nctx):
            ln = int(buf[p]); p += 1
            ctx.append(buf[p:p + 2 * ln].reshape(-1, 2).tolist()); p += 2 * ln
        calls.append(dict(agent=agent, goal=[tx, ty] if has else None, success=bool(ok), cost=cost, fmin=fmin, expanded=expanded,
                          decrease_keys=dk, vertex_constraints=vc, edge_constraints=ec, states=states, actions=actions,
                          action_costs=costs, ctx_paths=ctx))
    return dict(solved=bool(stats[0]), cost=int(stats[1]), hl_expanded=int(stats[2]), end=end.tolist()), calls
