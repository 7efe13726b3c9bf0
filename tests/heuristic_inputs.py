"""The (map, goal) inputs of the shortest-path table tests (tests/test_heuristic_emu_cpu.py on the emulator,
tests/test_heuristic_gpu.py on the device) and the plain BFS both compare with."""
import json
import os
from collections import deque

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = 2 ** 31 - 1


def bfs(dimx, dimy, obstacles, goal):
    """ShortestPathHeuristic::getValue(cell, goal) (example/shortest_path_heuristic.hpp:12-63) for every cell: one vertex
    per cell, an edge between two adjacent cells when both are free, d[v][v] = 0 for every vertex — so a goal on an
    obstacle is 0 there and unreachable (INT32_MAX) everywhere else."""
    blocked = np.zeros((dimy, dimx), dtype=bool)
    for o in obstacles:
        if 0 <= o[0] < dimx and 0 <= o[1] < dimy:
            blocked[o[1], o[0]] = True
    dist = np.full((dimy, dimx), INF, dtype=np.int64)
    dist[goal[1], goal[0]] = 0
    if blocked[goal[1], goal[0]]:
        return dist
    q = deque([(goal[0], goal[1])])
    while q:
        x, y = q.popleft()
        d = dist[y, x] + 1
        for nx, ny in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
            if 0 <= nx < dimx and 0 <= ny < dimy and not blocked[ny, nx] and dist[ny, nx] == INF:
                dist[ny, nx] = d
                q.append((nx, ny))
    return dist


def serpentine():
    """The map of tests/test_compact_emu.py::test_long_horizons: (0, 0) to (0, 12) is 198 steps."""
    obst = [[x, y] for y in range(1, 12, 2) for x in range(32) if x != (31 if (y // 2) % 2 == 0 else 0)]
    return dict(dimx=32, dimy=32, obstacles=obst)


def random_map(dimx, dimy, seed, density=0.2):
    rng = np.random.default_rng(seed)
    mask = rng.random((dimy, dimx)) < density
    return dict(dimx=dimx, dimy=dimy, obstacles=[[int(x), int(y)] for y, x in zip(*np.nonzero(mask))])


def free_cells(m):
    obst = {(o[0], o[1]) for o in m["obstacles"]}
    return [[x, y] for y in range(m["dimy"]) for x in range(m["dimx"]) if (x, y) not in obst]


def small_inputs():
    """(map, [goals]) for the maps up to 32 x 32."""
    with open(os.path.join(GOLDEN, "bench_instances.json")) as f:
        bench = json.load(f)
    with open(os.path.join(GOLDEN, "ref_tests.json")) as f:
        ref = json.load(f)
    out = []
    for name in sorted(bench):
        if name.startswith("map_8by8_") or name.startswith("map_32by32_"):
            inst = bench[name]
            out.append((dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"]),
                        sorted({tuple(g) for g in inst["goals"]})))
    for name in sorted(ref["cbs_ta"]["inputs"]):
        inst = ref["cbs_ta"]["inputs"][name]
        goals = sorted({tuple(g) for pg in inst["potential_goals"] for g in pg})
        out.append((dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"]), goals))
    out.append((serpentine(), [(0, 12), (0, 0), (31, 31), (5, 1)]))  # (5, 1) is a wall cell
    # a walled-off pocket: the cells inside x, y = 10 .. 13 are cut off from the rest
    pocket = [[x, y] for x in range(9, 15) for y in range(9, 15) if x in (9, 14) or y in (9, 14)]
    out.append((dict(dimx=20, dimy=17, obstacles=pocket + [[25, 3], [-1, 2]]), [(0, 0), (11, 11), (19, 16), (9, 9)]))
    out.append((dict(dimx=1, dimy=1, obstacles=[]), [(0, 0)]))
    out.append((dict(dimx=1, dimy=1, obstacles=[[0, 0]]), [(0, 0)]))
    out.append((dict(dimx=32, dimy=1, obstacles=[[7, 0]]), [(0, 0), (31, 0), (7, 0)]))
    out.append((dict(dimx=3, dimy=32, obstacles=[[1, y] for y in range(1, 31)]), [(0, 0), (2, 31), (1, 5)]))
    out.append((dict(dimx=31, dimy=29, obstacles=random_map(31, 29, 3)["obstacles"]), [(0, 0), (30, 28), (15, 14)]))
    return out


def large_inputs():
    """(map, [goals]) for the layout beyond 32 x 32 (stride dimx): corridors and seeded random maps, about 20 % obstacles;
    goals: the corners' nearest free cells, a few random free cells, one obstacle cell."""
    out = [(dict(dimx=1, dimy=40, obstacles=[]), [(0, 0), (0, 39), (0, 17)]),
           (dict(dimx=40, dimy=1, obstacles=[]), [(0, 0), (39, 0), (17, 0)]),
           (dict(dimx=40, dimy=1, obstacles=[[20, 0]]), [(3, 0), (20, 0), (39, 0)]),
           (dict(dimx=64, dimy=3, obstacles=[[x, 1] for x in range(1, 64)]), [(63, 0), (63, 2), (5, 1)])]
    for k, (dx, dy, ngoals) in enumerate(((33, 32, 6), (48, 48, 6), (100, 37, 6), (64, 64, 4), (255, 255, 4))):
        m = random_map(dx, dy, 100 + k)
        fc = free_cells(m)
        rng = np.random.default_rng(200 + k)
        goals = [tuple(fc[0]), tuple(fc[-1])] + [tuple(fc[int(i)]) for i in rng.integers(0, len(fc), ngoals - 3)]
        goals.append(tuple(m["obstacles"][len(m["obstacles"]) // 2]))
        out.append((m, goals))
    return out
