"""Corpus and references of the task-assignment solvers beyond 64 agents (tests/test_ta_wide_restatement_cpu.py,
test_cbs_ta_wide_driver_cpu.py, test_ecbs_ta_wide_driver_cpu.py on the CPU, test_cbs_ta_wide_gpu.py, test_ecbs_ta_wide_gpu.py on
the device).  CPU only: the engine is never imported.

reference(inst) runs tests/support/cbs_ta_tree_wide_check.cpp: cbs_ta_tree_check.cpp's sequential algorithm with masks of
mask_words words and the series over the WIDE assignment wave program on the CPU.  It takes any instance of up to 256 agents
and 256 tasks; on the narrow corpora it equals cbs_ta_corpus.reference field for field.

instance(seed, n_agents, n_pool): a 32 x 32 map with 100 obstacles; the agents start on distinct free cells, the pool is
n_pool distinct free cells, and every agent has 1 - 3 potential goals drawn from the six pool cells nearest its start
(Manhattan distance, ties by pool order), which keeps the conflict trees small.  INSTANCES names what each entry is for.
The seeds were chosen by running the restatement on the CPU; what it measured for them, CBS-TA, uncapped unless noted
(high-level expansions / roots created / popped roots with a conflict):
  a65 29 / 29 / 28, a80 50 / 50 / 49, a81 40 / 40 / 39, a96 23 / 23 / 22, fewer_tasks 41 / 41 / 40, more_tasks 77 / 77 / 76,
  cross 8 / 8 / 7, cross_back 42 / 42 / 41 (0.2 - 1.5 s each); a256_cap under the cap of 3 expansions: 3 / 4 / 3, 1030 searches, 3.3 s.
  a128 and a129 run under the same cap in CBS-TA: among the seeds tried for them (several hundred each, pools of 256 cells)
  none ended within 100 expansions — every root of 128 agents on this map has a conflict, and the next assignment costs no
  more than the children — so no solved CBS-TA answer above 96 agents is checked.  ECBS-TA (reference_ecbs, ecbs_named) at
  w = 1.3 solves both in 27 expansions (one root, 180 searches, 0.2 s), so there they run uncapped; at w = 1.0 most wide
  instances end in 3 - 41 expansions, more_tasks in 137, a128 / a129 not within 200 (capped as in CBS-TA).
validate(inst, result) is independent of both: tasks distinct and allowed, paths from start to task, no vertex or edge
conflict by getFirstConflict's definition (the step at which the longest path ends included), cost = sum of path costs."""
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

from cbs_ta_corpus import FIELDS, I32P, I64P, same  # noqa: E402,F401

# name: (seed, agents, pool cells, kind)   kind "cross": the tasks from index 64 on are allowed to agents below 64 only, and the
# agents from 64 on may take tasks below 64 only;  "cross_back": agents below 64 name fewer than 64 tasks, so tasks below 64 are
# allowed to agents from 64 on only;  "cap": run under max_hl_expansions = CAP_HL, ends MRP_HL_CAP
INSTANCES = {
    "a65": (1, 65, 80, ""),
    "a80": (37, 80, 90, ""),
    "a81": (9, 81, 200, ""),
    "a96": (26, 96, 230, ""),
    "a128": (0, 128, 256, "cap"),
    "a129": (0, 129, 256, "cap"),           # three mask words
    "fewer_tasks": (58, 70, 66, ""),     # 70 agents, 66 tasks: idle agents
    "more_tasks": (6, 66, 200, ""),
    "cross": (1, 72, 100, "cross"),
    "cross_back": (6, 72, 100, "cross_back"),
    "a256_cap": (0, 256, 256, "cap"),
}
CAP_HL = 3
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    import oracle
    oracle.build()
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, "libcbs_ta_tree_wide_check.so")
    sup = os.path.join(ROOT, "tests", "support")
    src = os.path.join(sup, "cbs_ta_tree_wide_check.cpp")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [src, os.path.join(sup, "ta_series_emu.h"), os.path.join(sup, "ta_series_emu_wide.h"), os.path.join(csrc, "assign_wave.h"),
            os.path.join(csrc, "assign_wave_wide.h"), os.path.join(csrc, "host", "assign_series.h"), os.path.join(csrc, "host", "assign_pack.h")]
    deps += [os.path.join(ROOT, "oracle", h) for h in os.listdir(os.path.join(ROOT, "oracle")) if h.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "oracle"), "-I", sup,
                               "-o", tmp, src])
        os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.cbs_ta_tree_wide_solve.restype = ctypes.c_int
    L.cbs_ta_tree_wide_solve.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, I32P, I32P, I32P, ctypes.c_int64,
                                         ctypes.c_int64, I64P, I32P, I32P]
    _lib = L
    return L


def reference(inst, max_task_assignments=2 ** 30, max_hl=-1):
    """The wide restatement's answer, in the form of cbs_ta_corpus.reference."""
    na = len(inst["starts"])
    ob = np.ascontiguousarray(np.asarray(inst["obstacles"], dtype=np.int32).reshape(-1, 2))
    st = np.ascontiguousarray(np.asarray(inst["starts"], dtype=np.int32).reshape(-1, 2))
    first = np.zeros(na + 1, dtype=np.int32)
    np.cumsum([len(g) for g in inst["potential_goals"]], out=first[1:])
    gl = np.ascontiguousarray(np.asarray([c for g in inst["potential_goals"] for c in g], dtype=np.int32).reshape(-1, 2))
    out = np.zeros(10, dtype=np.int64)
    tasks = np.zeros((max(na, 1), 2), dtype=np.int32)
    ends = np.zeros((max(na, 1), 3), dtype=np.int32)
    rc = lib().cbs_ta_tree_wide_solve(inst["dimx"], inst["dimy"], len(ob), ob.ctypes.data_as(I32P), na, st.ctypes.data_as(I32P),
                                      first.ctypes.data_as(I32P), gl.ctypes.data_as(I32P), max_task_assignments, max_hl,
                                      out.ctypes.data_as(I64P), tasks.ctypes.data_as(I32P), ends.ctypes.data_as(I32P))
    assert rc == 0
    r = dict(zip(FIELDS, (int(v) for v in out)))
    r["digest"] &= 2 ** 64 - 1
    solved = r["status"] == 0
    r["tasks"] = [None if tasks[a][0] < 0 else tasks[a].tolist() for a in range(na)] if solved else None
    r["ends"] = ends[:na].tolist() if solved else None
    return r


def instance(seed, n_agents, n_pool, kind=""):
    rng = random.Random(77000 + seed)
    cells = [(x, y) for y in range(32) for x in range(32)]
    obst = rng.sample(cells, 100)
    free = [c for c in cells if c not in set(obst)]
    starts = rng.sample(free, n_agents)
    pool = rng.sample(free, n_pool)
    goals = []
    for a, s in enumerate(starts):
        near = sorted(range(n_pool), key=lambda t: (abs(pool[t][0] - s[0]) + abs(pool[t][1] - s[1]), t))[:6]
        goals.append([pool[t] for t in rng.sample(near, rng.randint(1, 3))])
    if kind == "cross":
        # tasks are numbered in order of first appearance.  Agents 0 .. 63 name more than 64 tasks between them — those from index 64 on are allowed to agents
        # below 64 only (bits of mask word 1 in group 0) — and the agents from 64 on draw from tasks 0 .. 63 alone
        order = []
        for gs in goals[:64]:
            order.extend(g for g in gs if g not in order)
        assert len(order) > 64
        for a in range(64, n_agents):
            sx, sy = starts[a]
            near = sorted(range(64), key=lambda t: (abs(order[t][0] - sx) + abs(order[t][1] - sy), t))[:6]
            goals[a] = [order[t] for t in rng.sample(near, rng.randint(1, 3))]
    if kind == "cross_back":
        # agents 0 .. 63 draw from the first 40 pool cells only, so they name at most 40 tasks; the agents from 64 on draw from
        # the other cells: the tasks they name first get indices from there on, the first of them below 64 (mask word 0,
        # allowed to agents of group 1 only)
        for a, (sx, sy) in enumerate(starts):
            cand = range(40) if a < 64 else range(40, n_pool)
            near = sorted(cand, key=lambda t: (abs(pool[t][0] - sx) + abs(pool[t][1] - sy), t))[:6]
            goals[a] = [pool[t] for t in rng.sample(near, rng.randint(1, 3))]
    return dict(dimx=32, dimy=32, obstacles=[list(o) for o in obst], starts=[list(s) for s in starts],
                potential_goals=[[list(g) for g in gs] for gs in goals])


def named():
    """name -> (instance, max_hl_expansions)."""
    return {name: (instance(seed, na, npool, kind), CAP_HL if kind == "cap" else -1) for name, (seed, na, npool, kind) in INSTANCES.items()}


def ecbs_named(w):
    """name -> (instance, max_hl_expansions) for ECBS-TA under weight w: as named(), except that at w > 1 the 128- and 129-agent
    instances run uncapped — the restatement solves them in 27 expansions at w = 1.3 (two full and three mask words, solved
    to the end); the 256-agent one stays capped at every weight."""
    out = named()
    if w > 1.0:
        for name in ("a128", "a129"):
            out[name] = (out[name][0], -1)
    return out


def references():
    return {name: reference(inst, max_hl=cap) for name, (inst, cap) in named().items()}


_ecbs_lib = None
_ecbs_cache = {}


def ecbs_lib():
    global _ecbs_lib
    if _ecbs_lib is not None:
        return _ecbs_lib
    lib()  # (the oracle, the build directory)
    build = os.path.join(ROOT, "tests", "_build")
    out = os.path.join(build, "libecbs_ta_tree_wide_check.so")
    sup = os.path.join(ROOT, "tests", "support")
    src = os.path.join(sup, "ecbs_ta_tree_wide_check.cpp")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [src, os.path.join(sup, "ecbs_ta_check.cpp"), os.path.join(sup, "ta_series_emu.h"), os.path.join(sup, "ta_series_emu_wide.h"),
            os.path.join(csrc, "assign_wave.h"), os.path.join(csrc, "assign_wave_wide.h"), os.path.join(csrc, "host", "assign_series.h"),
            os.path.join(csrc, "host", "assign_pack.h")]
    deps += [os.path.join(ROOT, "oracle", h) for h in os.listdir(os.path.join(ROOT, "oracle")) if h.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "oracle"), "-I", sup,
                               "-o", tmp, src])
        os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.ecbs_ta_tree_wide_solve.restype = ctypes.c_int
    L.ecbs_ta_tree_wide_solve.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, I32P, I32P, I32P, ctypes.c_float,
                                          ctypes.c_int64, ctypes.c_int64, I64P, I32P, I32P, I32P, I32P, ctypes.c_int]
    _ecbs_lib = L
    return L


def reference_ecbs(inst, w, max_task_assignments=2 ** 30, max_hl=-1):
    """The wide ECBS-TA restatement's answer (tests/support/ecbs_ta_tree_wide_check.cpp), in the form of
    ecbs_ta_tree_corpus.reference; computed once per (instance, w, limits), callers leave it unchanged."""
    import ecbs_ta_tree_corpus as e
    key = (repr(inst), float(w), max_task_assignments, max_hl)
    if key in _ecbs_cache:
        return _ecbs_cache[key]
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
    pxy = np.zeros((max(na, 1), e.PATH_CAP, 2), dtype=np.int32)
    rc = ecbs_lib().ecbs_ta_tree_wide_solve(inst["dimx"], inst["dimy"], len(ob), ob.ctypes.data_as(I32P), na, st.ctypes.data_as(I32P),
                                            first.ctypes.data_as(I32P), gl.ctypes.data_as(I32P), w, max_task_assignments, max_hl,
                                            out.ctypes.data_as(I64P), tasks.ctypes.data_as(I32P), ends.ctypes.data_as(I32P),
                                            plen.ctypes.data_as(I32P), pxy.ctypes.data_as(I32P), e.PATH_CAP)
    assert rc == 0 and int(plen.max()) <= e.PATH_CAP
    r = dict(zip(e.FIELDS, (int(v) for v in out[:10])))
    r["digest"] &= 2 ** 64 - 1
    r["reached"] = dict(zip(e.REACHED, (int(v) for v in out[10:])))
    solved = r["status"] == 0
    r["tasks"] = [None if tasks[a][0] < 0 else tasks[a].tolist() for a in range(na)] if solved else None
    r["ends"] = ends[:na].tolist() if solved else None
    r["paths_xy"] = [pxy[a, :plen[a]].tolist() for a in range(na)] if solved else None
    _ecbs_cache[key] = r
    return r


def validate(inst, got):
    """An independent check of a SOLVED answer (hl.solve_cbs_ta_batch / solve_ecbs_ta_batch result `got`)."""
    na = len(inst["starts"])
    obst = {tuple(o) for o in inst["obstacles"]}
    tasks = got["tasks"]
    taken = [tuple(t) for t in tasks if t is not None]
    assert len(taken) == len(set(taken)), "tasks pairwise distinct"
    paths = got["paths"]
    assert len(paths) == na
    cost = 0
    for a in range(na):
        p = paths[a]
        assert [p[0][0], p[0][1]] == list(inst["starts"][a]), ("starts at its start", a)
        if tasks[a] is not None:
            assert list(tasks[a]) in [list(g) for g in inst["potential_goals"][a]], ("task among the potential goals", a)
            assert [p[-1][0], p[-1][1]] == list(tasks[a]), ("ends on its task", a)
        for k, (x, y, t) in enumerate(p):
            assert 0 <= x < inst["dimx"] and 0 <= y < inst["dimy"] and (x, y) not in obst, (a, k)
            if k:
                assert abs(x - p[k - 1][0]) + abs(y - p[k - 1][1]) <= 1, ("a step or a wait", a, k)
        cost += p[-1][2]
    assert cost == got["cost"], "cost = sum of path costs"
    longest = max(len(p) for p in paths)
    at = lambda p, t: (p[min(t, len(p) - 1)][0], p[min(t, len(p) - 1)][1])  # noqa: E731
    for t in range(longest):  # getFirstConflict: t = 0 .. longest - 1, the last step included
        seen = {}
        for a in range(na):
            c = at(paths[a], t)
            assert c not in seen, ("vertex conflict", t, seen.get(c), a)
            seen[c] = a
        moves = {}
        for a in range(na):
            moves[(at(paths[a], t), at(paths[a], t + 1))] = a
        for (u, v), a in moves.items():
            assert u == v or (v, u) not in moves, ("edge conflict", t, a, moves.get((v, u)))
