"""Corpus and reference of the CBS-TA conflict tree (tests/test_cbs_ta_tree_cpu.py, test_cbs_ta_driver_cpu.py on the CPU,
test_cbs_ta_gpu.py on the device).  CPU only: the engine is never imported.

reference(inst) runs tests/support/cbs_ta_tree_check.cpp — the sequential restatement of cbs_ta.hpp:87-214 with the
Environment's assignment bookkeeping over the oracle's low level — and returns what a driver's answer is compared with.
The seeded instances are small on purpose: 5 x 5 .. 8 x 8, 2 - 5 agents, potential goals drawn from a shared pool so that
they overlap, sometimes fewer goals than agents; SEEDS was chosen by running the restatement (the counts the tests assert:
at least a third of the instances expand a root that has a conflict, at least five create three or more roots)."""
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

I32P = ctypes.POINTER(ctypes.c_int32)
I64P = ctypes.POINTER(ctypes.c_int64)
FIELDS = ("status", "cost", "makespan", "hl_expanded", "ll_expanded", "num_task_assignments", "n_roots", "root_conflicts",
          "digest", "n_ll_searches")
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
         33, 34, 37, 50, 83, 93, 94)
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    import oracle
    oracle.build()
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, "libcbs_ta_tree_check.so")
    sup = os.path.join(ROOT, "tests", "support")
    src = os.path.join(sup, "cbs_ta_tree_check.cpp")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [src, os.path.join(sup, "ta_series_emu.h"), os.path.join(csrc, "assign_wave.h"), os.path.join(csrc, "host", "assign_series.h"),
            os.path.join(csrc, "host", "assign_pack.h")] + [os.path.join(ROOT, "oracle", h) for h in os.listdir(os.path.join(ROOT, "oracle"))
                                                            if h.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "oracle"), "-I", sup,
                               "-o", tmp, src])
        os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.cbs_ta_tree_solve.restype = ctypes.c_int
    L.cbs_ta_tree_solve.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, I32P, I32P, I32P, ctypes.c_int64,
                                    ctypes.c_int64, I64P, I32P, I32P]
    _lib = L
    return L


def reference(inst, max_task_assignments=2 ** 30, max_hl=-1):
    """The restatement's answer: FIELDS, tasks (per agent [x, y] or None) and ends (per agent [x, y, t])."""
    na = len(inst["starts"])
    ob = np.ascontiguousarray(np.asarray(inst["obstacles"], dtype=np.int32).reshape(-1, 2))
    st = np.ascontiguousarray(np.asarray(inst["starts"], dtype=np.int32).reshape(-1, 2))
    first = np.zeros(na + 1, dtype=np.int32)
    np.cumsum([len(g) for g in inst["potential_goals"]], out=first[1:])
    gl = np.ascontiguousarray(np.asarray([c for g in inst["potential_goals"] for c in g], dtype=np.int32).reshape(-1, 2))
    out = np.zeros(10, dtype=np.int64)
    tasks = np.zeros((max(na, 1), 2), dtype=np.int32)
    ends = np.zeros((max(na, 1), 3), dtype=np.int32)
    rc = lib().cbs_ta_tree_solve(inst["dimx"], inst["dimy"], len(ob), ob.ctypes.data_as(I32P), na, st.ctypes.data_as(I32P),
                                 first.ctypes.data_as(I32P), gl.ctypes.data_as(I32P), max_task_assignments, max_hl,
                                 out.ctypes.data_as(I64P), tasks.ctypes.data_as(I32P), ends.ctypes.data_as(I32P))
    assert rc == 0
    r = dict(zip(FIELDS, (int(v) for v in out)))
    r["digest"] &= 2 ** 64 - 1
    solved = r["status"] == 0
    r["tasks"] = [None if tasks[a][0] < 0 else tasks[a].tolist() for a in range(na)] if solved else None
    r["ends"] = ends[:na].tolist() if solved else None
    return r


def same(got, ref):
    """A driver's result (hl.solve_cbs_ta_batch) against the restatement's: status, cost, both counters, the assignments
    asked for, tasks, schedule digest, and the bookkeeping beside them."""
    for f in FIELDS:
        assert got[f] == ref[f], (f, got[f], ref[f])
    assert got["tasks"] == ref["tasks"]
    if ref["ends"] is not None:
        assert [p[-1] for p in got["paths"]] == ref["ends"]


def instance(seed):
    rng = random.Random(9000 + seed)
    dim = rng.randint(5, 8)
    cells = [(x, y) for y in range(dim) for x in range(dim)]
    obst = rng.sample(cells, rng.randint(0, dim))
    free = [c for c in cells if c not in set(obst)]
    na = rng.randint(2, 5)
    starts = rng.sample(free, na)
    pool = rng.sample(free, rng.randint(max(1, na - 1), na + 2))  # sometimes fewer goals than agents
    goals = [rng.sample(pool, rng.randint(1, min(3, len(pool)))) for _ in range(na)]
    return dict(dimx=dim, dimy=dim, obstacles=[list(o) for o in obst], starts=[list(s) for s in starts],
                potential_goals=[[list(g) for g in gs] for gs in goals])


def corpus():
    return [instance(s) for s in SEEDS]


def ref_inputs(ref_tests):
    out = {}
    for name, inst in sorted(ref_tests["cbs_ta"]["inputs"].items()):
        out[name] = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"], starts=inst["starts"],
                         potential_goals=inst["potential_goals"])
    return out
