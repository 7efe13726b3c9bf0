"""The shortest-path table program (libmultirobotplanning_amd/csrc/heur_bfs.h — the source the gfx950 kernel compiles)
on the CPU: the same file built against tests/support/wave_emu_heur.h, the 64-lane lockstep interpretation of its wave
vocabulary, one table per call.  Every table must equal a plain deque BFS (tests/heuristic_inputs.py) cell for cell, with
no LDS access outside the window the host asks the launch for and no word changed outside the table."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import heuristic_inputs as hi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = ctypes.POINTER(ctypes.c_int32)
I64P = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def emu():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    sanitize = bool(os.environ.get("MRP_EMU_SANITIZE"))
    lib = os.path.join(build, "libemu_heur%s.so" % ("_san" if sanitize else ""))
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [os.path.join(ROOT, "tests", "support", "emu_heur.cpp"), os.path.join(ROOT, "tests", "support", "wave_emu_heur.h"),
            os.path.join(ROOT, "tests", "support", "wave_emu.h"), os.path.join(csrc, "heur_bfs.h"),
            os.path.join(csrc, "heur_layout.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-Wall"] + san + ["-o", lib, deps[0]])
    L = ctypes.CDLL(lib)
    L.emu_heuristic_table.restype = ctypes.c_int
    L.emu_heuristic_table.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, ctypes.c_int, I32P, I64P]
    return L


def _table(L, m, goal):
    obst = np.ascontiguousarray(np.asarray(m["obstacles"], dtype=np.int32).reshape(-1, 2))
    dist = np.zeros((m["dimy"], m["dimx"]), dtype=np.int32)
    out = np.zeros(4, dtype=np.int64)
    rc = L.emu_heuristic_table(m["dimx"], m["dimy"], len(obst), obst.ctypes.data_as(I32P), goal[0], goal[1],
                               dist.ctypes.data_as(I32P), out.ctypes.data_as(I64P))
    assert rc == 0, rc
    assert out[0] == 0 and out[1] == 0, ("LDS access outside the window", m["dimx"], m["dimy"], goal, out.tolist())
    assert out[2] == 0, ("words outside the table changed", m["dimx"], m["dimy"], goal)
    return dist, int(out[3])


def _check(L, inputs):
    n = 0
    for m, goals in inputs:
        for g in goals:
            got, _ = _table(L, m, g)
            want = hi.bfs(m["dimx"], m["dimy"], m["obstacles"], g)
            assert np.array_equal(got, want), (m["dimx"], m["dimy"], g, np.argwhere(got != want)[:5].tolist())
            n += 1
    return n


def test_small_maps_every_table_equals_bfs(emu):
    """Every agent goal of the shipped 8 x 8 and 32 x 32 instances, every potential goal of the reference's cbs_ta
    fixtures, the 198-step serpentine, a walled-off pocket, goals on obstacles, 1 x 1, rows and columns."""
    inputs = hi.small_inputs()
    far = hi.bfs(32, 32, hi.serpentine()["obstacles"], (0, 12))
    assert far[0, 0] == 198
    assert _check(emu, inputs) >= 200


def test_large_maps_every_table_equals_bfs(emu):
    """The layout beyond 32 x 32 (halfword [y * dimx + x]): 1 x 40 and 40 x 1 corridors, 33 x 32, 48 x 48, 100 x 37, 64 x 64
    (dimx a multiple of 32: whole-word row shifts) and 255 x 255 with about 20 % random obstacles."""
    inputs = hi.large_inputs()
    assert {(m["dimx"], m["dimy"]) for m, _ in inputs} >= {(1, 40), (40, 1), (33, 32), (48, 48), (100, 37), (255, 255)}
    assert _check(emu, inputs) >= 30


def test_special_cases(emu):
    """A goal on an obstacle: 0 there, unreachable everywhere else (Floyd-Warshall's d[v][v] = 0).  A pocket: unreachable
    from outside, reachable inside.  The window is what heur_layout.h says: 2 KB for the small form, 40 KB at 255 x 255."""
    m = hi.serpentine()
    got, lds = _table(emu, m, (5, 1))
    assert lds == 2048 and got[1, 5] == 0 and (got == hi.INF).sum() == 32 * 32 - 1
    m, goals = [x for x in hi.small_inputs() if x[0]["dimx"] == 20][0]
    outside, _ = _table(emu, m, (0, 0))
    inside, _ = _table(emu, m, (11, 11))
    assert outside[11, 11] == hi.INF and inside[0, 0] == hi.INF and inside[13, 13] == 4 and outside[16, 19] == 35
    big = hi.random_map(255, 255, 104)
    _, lds = _table(emu, big, tuple(hi.free_cells(big)[0]))
    assert lds == 5 * 4 * 2048
