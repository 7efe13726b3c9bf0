"""The compact tier's search with its focal path table in device memory (PLDS = false: what the front workgroups of
mrp_ll_session_front_tables run) against the same search with the table behind the LDS window (PLDS = true), on the CPU
emulator of the wave vocabulary (tests/support/wave_emu.h; the search is the kernels' own source, csrc/ll_compact.h).

tests/support/emu_front_tables.cpp runs chain-shaped sequences: one search per agent of an instance, each against the paths
found before it — with the root chain's table [64][npad] (rows = 64) and with a conflict-tree child's table, which has as many
rows as the longest earlier path has cells (rows = 0: the search clamps to row tPad - 1).  Both placements of the table must
give, search by search, the same result record, the same path and the same final words of the open and the focal area of the
window; neither may touch a byte outside its window, which in memory mode ends where the table used to begin."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import root_chain_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P, I64P, U32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32)
HEAP_WORDS = 2 * (1024 * 4 + 16) // 4  # ll_compact.h: the open and the focal area of the narrow window, Narrow::kHeapBytes each
C_OK, C_CAP_EXP = 0, 2


@pytest.fixture(scope="module")
def emu():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    lib = os.path.join(build, "libemu_front_tables.so")
    deps = [os.path.join(ROOT, "tests", "support", "emu_front_tables.cpp"), os.path.join(ROOT, "tests", "support", "wave_emu.h"),
            os.path.join(ROOT, "libmultirobotplanning_amd", "csrc", "ll_compact.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", lib, deps[0]])
    L = ctypes.CDLL(lib)
    L.emu_front_chain.restype = ctypes.c_int
    L.emu_front_chain.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P, ctypes.c_int, I32P,
                                  ctypes.c_float, ctypes.c_int64, I64P, I32P, U32P, ctypes.c_int]
    return L


def run(L, in_memory, rows, inst, w, budget=-1):
    n = len(inst["starts"])
    obst = np.ascontiguousarray(np.asarray(inst["obstacles"], dtype=np.int32).reshape(-1, 2))
    sg = np.ascontiguousarray(np.asarray([s + g for s, g in zip(inst["starts"], inst["goals"])], dtype=np.int32))
    out = np.full((n, 8), -99, dtype=np.int64)
    cells = np.full((n, 64), -99, dtype=np.int32)
    heaps = np.zeros((n, HEAP_WORDS), dtype=np.uint32)
    done = L.emu_front_chain(in_memory, rows, inst["dimx"], inst["dimy"], len(obst), obst.ctypes.data_as(I32P), n,
                             sg.ctypes.data_as(I32P), w, budget, out.ctypes.data_as(I64P), cells.ctypes.data_as(I32P),
                             heaps.ctypes.data_as(U32P), HEAP_WORDS)
    assert done >= 0, done
    return done, out[:done], cells[:done], heaps[:done]


def both(L, rows, inst, w, budget=-1):
    """The sequence with the table in the window and in memory: equal in everything; returns the former's (done, out, cells)."""
    d0, o0, c0, h0 = run(L, 0, rows, inst, w, budget)
    d1, o1, c1, h1 = run(L, 1, rows, inst, w, budget)
    assert d0 == d1
    assert np.array_equal(o0, o1), np.argwhere(o0 != o1)[:4]   # status, cost, fmin, n_states, expanded, nodes, stray accesses
    assert np.array_equal(c0, c1)                                 # the paths
    assert np.array_equal(h0, h1), np.argwhere(h0 != h1)[:4]     # the open and the focal area as every search left them
    assert not o0[:, 6:].any()                                    # no LDS access outside the window, in either placement
    return d0, o0, c0


def near_instance(n, seed):
    """n agents on a 32 x 32 map with 60 obstacles; every goal within five cells of its start in x and y: short searches."""
    rng = np.random.RandomState(7000 + 13 * n + seed)
    cells = rng.permutation(32 * 32)
    blocked = {int(c) for c in cells[:60]}
    free = [int(c) for c in cells[60:]]
    starts, goals, used = [], [], set()
    for c in free:
        if len(starts) == n:
            break
        x, y = c % 32, c // 32
        for _ in range(20):
            gx, gy = x + int(rng.randint(-5, 6)), y + int(rng.randint(-5, 6))
            g = gy * 32 + gx
            if 0 <= gx < 32 and 0 <= gy < 32 and g not in blocked and g not in used:
                used.add(g)
                starts.append([x, y])
                goals.append([gx, gy])
                break
    assert len(starts) == n
    return dict(dimx=32, dimy=32, obstacles=[[c % 32, c // 32] for c in sorted(blocked)], starts=starts, goals=goals)


@pytest.mark.parametrize("rows", [64, 0])
@pytest.mark.parametrize("n", [1, 2, 10, 16, 17, 64, 65, 128])
def test_table_in_memory_equals_table_in_the_window(emu, n, rows):
    """1 .. 64 agents: one row load per table row (and, at 1, 2, 10 and 17, padded columns behind the last agent); 65 and 128:
    two.  Every search of the sequence has a path (the sequence runs to its end)."""
    inst = near_instance(n, 0)
    done, out, _ = both(emu, rows, inst, 1.3)
    assert done == n and (out[:, 0] == C_OK).all(), out[:, 0]
    assert out[:, 4].sum() > n  # (searches, not starts on goals)


def test_the_chain_form_is_the_oracles_chain(emu, oracle_mod):
    """Anchor: the ten-agent sequence with the chain's table is tests/root_chain_cases.py's model of that root chain."""
    inst = near_instance(10, 0)
    done, out, cells = both(emu, 64, inst, 1.3)
    model = rc.chain_model(inst, 1.3)
    assert done == 10 == model["n_states"]
    for a, r in enumerate(model["results"]):
        assert (r["status"], r["cost"], r["fmin"], r["n_states"], r["expanded"]) == tuple(int(v) for v in out[a, :5]), a
        assert [[int(c) & 0xFF, int(c) >> 8] for c in cells[a, :r["n_states"]]] == [s[1:] for s in r["states"]], a


def corridor():
    """A 32 x 3 map whose middle row is a wall but for its last cell: the way from (0, 0) to (2, 2) is along row 0, through
    (31, 1) and back along row 2 — 62 steps, 63 states, the longest path the tier holds.  Two short agents first, then the long
    one, then a short one behind it: the long search runs against tables of 4 rows (child form: it reads row tPad - 1 from
    t = 3 on), the last one against the long path."""
    return dict(dimx=32, dimy=3, obstacles=[[x, 1] for x in range(31)],
                starts=[[5, 0], [20, 2], [0, 0], [10, 2]], goals=[[8, 0], [18, 2], [2, 2], [12, 2]])


@pytest.mark.parametrize("rows", [64, 0])
def test_a_62_step_path_beside_shorter_ones(emu, rows):
    done, out, cells = both(emu, rows, corridor(), 1.0)
    assert done == 4 and (out[:, 0] == C_OK).all()
    assert [int(v) for v in out[:, 3]] == [4, 3, 63, 3]
    assert int(cells[2, 62]) == (2 | (2 << 8)) and int(cells[2, 32]) == (31 | (1 << 8))


@pytest.mark.parametrize("rows", [64, 0])
def test_an_expansion_cap_that_ends_mid_chain(emu, rows):
    """The budget covers the searches in front of agent k and three expansions of agent k's (k: the first agent from the fourth
    on whose search needs more than four): it ends as the cap does, after four expansions (the cap is looked at behind the
    expansion that exceeds it, as in the reference), and nothing behind it runs."""
    inst = near_instance(10, 0)
    _, whole, _ = both(emu, rows, inst, 1.3)
    k = next(a for a in range(3, 10) if int(whole[a, 4]) > 4)
    done, out, _ = both(emu, rows, inst, 1.3, budget=int(whole[:k, 4].sum()) + 3)
    assert done == k + 1
    assert np.array_equal(out[:k], whole[:k])
    assert (int(out[k, 0]), int(out[k, 4])) == (C_CAP_EXP, 4)
