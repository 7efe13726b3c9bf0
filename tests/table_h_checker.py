"""Loader of tests/support/table_h_check.cpp: the CPU truth for MRP_LL_JOB_TABLE_H — the oracle's AStar / AStarEpsilon over
the oracle's grid Environment with admissibleHeuristic read from a table the test passes in.  Built from the oracle's
headers into tests/_build/ on first use: as a shared library for ctypes, and (sanitized_program) as a stand-alone program
under -fsanitize=address,undefined that runs a file of cases."""
import ctypes
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "support", "table_h_check.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "oracle", h) for h in ("search_restated.hpp", "mapf_restated.hpp", "heap_restated.hpp")]
I32P = ctypes.POINTER(ctypes.c_int32)
I64P = ctypes.POINTER(ctypes.c_int64)
_lib = None


def _build(out, flags):
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "oracle")] + flags + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(_build(os.path.join(BUILD, "libtable_h_check.so"), ["-O2", "-fPIC", "-shared"]))
        L.table_h_ll_search.restype = ctypes.c_int
        L.table_h_ll_search.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_int] * 2 + [ctypes.c_int, I32P] + [ctypes.c_int] * 5 + \
            [I32P, ctypes.c_int, I32P, ctypes.c_int, I32P, ctypes.c_int, I32P, I32P, ctypes.c_int64, ctypes.c_int, I32P, I64P, I32P,
             I32P, ctypes.c_int]
        _lib = L
    return _lib


def sanitized_program():
    """The same source with its own main, under the host sanitizers (nothing of it is ever loaded into Python)."""
    return _build(os.path.join(BUILD, "table_h_check_san"),
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DTABLE_H_CHECK_MAIN"])


def _i32(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(shape))
    return a, a.ctypes.data_as(I32P)


def ll_search(algo, inst_map, start, goal, table, vertex_constraints=(), edge_constraints=(), w=1.0, agent_idx=0, ctx_paths=(),
              cap_expansions=-1, initial_cost=0, cap=2048):
    """One low-level search with h = table[y][x] (INT32_MAX: unreachable).  algo 0 = AStar, 1 = AStarEpsilon.  Returns what
    oracle.ll_search returns: rc (-1: expansion cap), success, cost, fmin, expanded, states [t, x, y], actions."""
    obst, obst_p = _i32(inst_map["obstacles"], (-1, 2))
    tab, tab_p = _i32(table, (inst_map["dimy"], inst_map["dimx"]))
    vc, vc_p = _i32(vertex_constraints, (-1, 3))
    ec, ec_p = _i32(edge_constraints, (-1, 5))
    plen, plen_p = _i32([len(p) for p in ctx_paths], (-1,))
    pxy, pxy_p = _i32([xy for p in ctx_paths for xy in p], (-1, 2))
    out = np.zeros(4, dtype=np.int32)
    expanded = np.zeros(1, dtype=np.int64)
    states = np.zeros((cap, 3), dtype=np.int32)
    actions = np.zeros(cap, dtype=np.int32)
    rc = lib().table_h_ll_search(algo, w, inst_map["dimx"], inst_map["dimy"], len(obst), obst_p, agent_idx, start[0], start[1],
                                 goal[0], goal[1], tab_p, len(vc), vc_p, len(ec), ec_p, len(plen), plen_p, pxy_p, cap_expansions,
                                 initial_cost, out.ctypes.data_as(I32P), expanded.ctypes.data_as(I64P),
                                 states.ctypes.data_as(I32P), actions.ctypes.data_as(I32P), cap)
    n = int(out[3])
    assert n <= cap
    return dict(rc=rc, success=bool(out[0]), cost=int(out[1]), fmin=int(out[2]), expanded=int(expanded[0]),
                states=states[:n].tolist(), actions=actions[:max(n - 1, 0)].tolist())


def case_file_text(runs):
    """The stand-alone program's input for runs = [(algo, case)] (cases as tests/table_h_cases.py makes them)."""
    words = [len(runs)]
    for algo, c in runs:
        m = c["map"]
        w_bits = struct.unpack("<I", struct.pack("<f", c["w"]))[0]
        ctx = c["ctx"] if algo == 1 else []
        words += [algo, w_bits, m["dimx"], m["dimy"], c["agent"], c["start"][0], c["start"][1], c["goal"][0], c["goal"][1],
                  c["cap"], c["initial_cost"] if algo == 0 else 0, len(m["obstacles"]), len(c["vc"]), len(c["ec"]), len(ctx)]
        words += [v for o in m["obstacles"] for v in o]
        words += [int(v) for v in np.asarray(c["table"]).reshape(-1)]
        words += [v for x in c["vc"] for v in x] + [v for x in c["ec"] for v in x]
        words += [len(p) for p in ctx] + [v for p in ctx for xy in p for v in xy]
    return " ".join(str(int(v)) for v in words) + "\n"


def parse_program_line(line):
    v = [int(x) for x in line.split()]
    rc, ok, cost, fmin, n, expanded = v[:6]
    states = [v[6 + 3 * k:9 + 3 * k] for k in range(n)]
    actions = v[6 + 3 * n:6 + 3 * n + max(n - 1, 0)]
    return dict(rc=rc, success=bool(ok), cost=cost, fmin=fmin, expanded=expanded, states=states, actions=actions)
