"""Corpus and reference of the ECBS-TA conflict tree (tests/test_ecbs_ta_tree_cpu.py, test_ecbs_ta_driver_cpu.py on the CPU,
test_ecbs_ta_gpu.py on the device).  CPU only: the engine is never imported.

reference(inst, w) runs tests/support/ecbs_ta_tree_check.cpp — the sequential restatement of ecbs_ta.hpp:94-352 with the
Environment's assignment bookkeeping over the checker's AStarEpsilon low level — and returns what a driver's answer is
compared with, plus what the run reached (`reached`: expanded nodes with a conflict, roots that failed part-way, failed child
searches, an empty first assignment, new-root attempts).
The seeded instances are small on purpose: 5 x 5 .. 8 x 8, 2 - 5 agents, potential goals drawn from a shared pool so that
they overlap, sometimes fewer goals than agents, sometimes walled-in or unreachable goals; every instance is used with
w in WS.  SEEDS was chosen by running the restatement; the counts it was chosen for are asserted by
test_ecbs_ta_tree_cpu.py::test_the_corpus_reaches_what_it_is_for."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from cbs_ta_corpus import ref_inputs  # noqa: E402,F401  (the three reference inputs, shared with CBS-TA)

I32P = ctypes.POINTER(ctypes.c_int32)
I64P = ctypes.POINTER(ctypes.c_int64)
FIELDS = ("status", "cost", "makespan", "hl_expanded", "ll_expanded", "num_task_assignments", "n_roots", "root_conflicts",
          "digest", "n_ll_searches")
REACHED = ("conflict_nodes", "roots_failed_part_way", "child_failures", "first_assignment_empty", "root_attempts")
WS = (1.0, 1.3, 2.0)
PATH_CAP = 256
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 23, 27, 34, 40, 42, 44, 52, 53, 59, 61, 65, 69, 78, 90, 94, 97,
         102, 103, 106, 110, 111, 119, 121, 130, 138, 277)
_lib = None
_cache = {}


def lib():
    global _lib
    if _lib is not None:
        return _lib
    import oracle
    oracle.build()
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, "libecbs_ta_tree_check.so")
    sup = os.path.join(ROOT, "tests", "support")
    src = os.path.join(sup, "ecbs_ta_tree_check.cpp")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [src, os.path.join(sup, "ecbs_ta_check.cpp"), os.path.join(sup, "ta_series_emu.h"), os.path.join(csrc, "assign_wave.h"),
            os.path.join(csrc, "host", "assign_series.h"), os.path.join(csrc, "host", "assign_pack.h")]
    deps += [os.path.join(ROOT, "oracle", h) for h in os.listdir(os.path.join(ROOT, "oracle")) if h.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "oracle"), "-I", sup,
                               "-o", tmp, src])
        os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.ecbs_ta_tree_solve.restype = ctypes.c_int
    L.ecbs_ta_tree_solve.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, I32P, I32P, I32P, ctypes.c_float,
                                     ctypes.c_int64, ctypes.c_int64, I64P, I32P, I32P, I32P, I32P, ctypes.c_int]
    _lib = L
    return L


def reference(inst, w, max_task_assignments=2 ** 30, max_hl=-1):
    """The restatement's answer: FIELDS, tasks (per agent [x, y] or None), ends (per agent [x, y, t]), paths_xy and `reached`.  Computed
    once per (instance, w, limits) and shared: callers leave it unchanged."""
    key = (repr(inst), float(w), max_task_assignments, max_hl)
    if key in _cache:
        return _cache[key]
    na = len(inst["starts"])
    ob = np.ascontiguousarray(np.asarray(inst["obstacles"], dtype=np.int32).reshape(-1, 2))
    st = np.ascontiguousarray(np.asarray(inst["starts"], dtype=np.int32).reshape(-1, 2))
    first = np.zeros(na + 1, dtype=np.int32)
    np.cumsum([len(g) for g in inst["potential_goals"]], out=first[1:])
    gl = np.ascontiguousarray(np.asarray([c for g in inst["potential_goals"] for c in g], dtype=np.int32).reshape(-1, 2))
    out = np.zeros(15, dtype=np.int64)
    tasks = np.zeros((max(na, 1), 2), dtype=np.int32)
    ends = np.zeros((max(na, 1), 3), dtype=np.int32)
    plen = np.zeros(max(na, 1), dtype=np.int32)
    pxy = np.zeros((max(na, 1), PATH_CAP, 2), dtype=np.int32)
    rc = lib().ecbs_ta_tree_solve(inst["dimx"], inst["dimy"], len(ob), ob.ctypes.data_as(I32P), na, st.ctypes.data_as(I32P),
                                  first.ctypes.data_as(I32P), gl.ctypes.data_as(I32P), w, max_task_assignments, max_hl,
                                  out.ctypes.data_as(I64P), tasks.ctypes.data_as(I32P), ends.ctypes.data_as(I32P),
                                  plen.ctypes.data_as(I32P), pxy.ctypes.data_as(I32P), PATH_CAP)
    assert rc == 0 and int(plen.max()) <= PATH_CAP
    r = dict(zip(FIELDS, (int(v) for v in out[:10])))
    r["digest"] &= 2 ** 64 - 1
    r["reached"] = dict(zip(REACHED, (int(v) for v in out[10:])))
    solved = r["status"] == 0
    r["tasks"] = [None if tasks[a][0] < 0 else tasks[a].tolist() for a in range(na)] if solved else None
    r["ends"] = ends[:na].tolist() if solved else None
    r["paths_xy"] = [pxy[a, :plen[a]].tolist() for a in range(na)] if solved else None
    _cache[key] = r
    return r


def same(got, ref):
    """A driver's result (hl.solve_ecbs_ta_batch) against the restatement's: status, cost, makespan, both counters, the
    assignments asked for, roots, tasks, schedule digest and end states."""
    for f in FIELDS:
        assert got[f] == ref[f], (f, got[f], ref[f])
    assert got["tasks"] == ref["tasks"]
    if ref["ends"] is not None:
        assert [p[-1] for p in got["paths"]] == ref["ends"]


def instance(seed):
    rng = random.Random(77000 + seed)
    dim = rng.randint(5, 8)
    cells = [(x, y) for y in range(dim) for x in range(dim)]
    obst = rng.sample(cells, rng.randint(0, dim + 2))
    blocked = set(obst)
    free = [c for c in cells if c not in blocked]
    na = rng.randint(2, 5)
    starts = rng.sample(free, na)
    kind = rng.random()
    if kind < 0.08:  # nobody can be assigned anything: the first assignment is empty, the first root is planned taskless
        goals = [rng.sample(obst, min(len(obst), 1)) if obst else [] for _ in range(na)]
    else:
        pool = rng.sample(free, rng.randint(max(1, na - 1), na + 2))  # sometimes fewer goals than agents
        goals = [rng.sample(pool, rng.randint(1, min(3, len(pool)))) for _ in range(na)]
    return dict(dimx=dim, dimy=dim, obstacles=[list(o) for o in obst], starts=[list(s) for s in starts],
                potential_goals=[[list(g) for g in gs] for gs in goals])


def corpus():
    return [instance(s) for s in SEEDS]


def pairs():
    """Every (instance, w) of the corpus."""
    return [(i, w) for i in corpus() for w in WS]
