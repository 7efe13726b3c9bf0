"""Shared inputs and independent oracles of the assignment tests (pure Python and numpy).

A problem is a dict: nA, nT, cost (int64 array [nA][nT], NO_EDGE where there is no edge), forbidden (per agent a bit mask
of tasks, or None), mode (per agent FREE, a forced task >= 0, NO_TASK or SOME_TASK, or None) and min_matching.
The contract (assignment.hpp:81-118, next_best_assignment.hpp:49-189): a matching of maximum cardinality and, among
those, of minimum total cost, under the constraints; the series is every matching of the optimum's cardinality K, once,
in non-decreasing order of cost."""
import json
import os

import numpy as np

import heuristic_inputs as hi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

NO_EDGE = 2 ** 31 - 1
MAX_COST = 2 ** 24 - 1
FREE, NO_TASK, SOME_TASK = -1, -2, -3
OK, INFEASIBLE, BAD_JOB = 0, 1, 5  # MRP_LL_OK, MRP_LL_NO_SOLUTION, MRP_LL_BAD_JOB


def problem(cost, forbidden=None, mode=None, min_matching=0):
    c = np.asarray(cost, dtype=np.int64)
    assert c.ndim == 2
    return dict(nA=c.shape[0], nT=c.shape[1], cost=c, forbidden=None if forbidden is None else [int(f) for f in forbidden],
                mode=None if mode is None else [int(m) for m in mode], min_matching=int(min_matching))


def allowed_pair(p, a, t):
    """May agent a take task t (t = -1: none) under the problem's edges and constraints?"""
    m = FREE if p["mode"] is None else p["mode"][a]
    if t < 0:
        return m in (FREE, NO_TASK)
    if p["cost"][a, t] == NO_EDGE:
        return False
    if p["forbidden"] is not None and (p["forbidden"][a] >> t) & 1:
        return False
    return m in (FREE, SOME_TASK) or m == t


def brute(p):
    """Every agent -> task-or-none map that honours the constraints.  Returns (K, optimal cost, sorted list of
    (cost, matching) at cardinality K) — (None, None, []) when the problem is infeasible."""
    nA, nT = p["nA"], p["nT"]
    found = []  # (pairs, cost, matching)
    cur = [-1] * nA

    def rec(a, used, pairs, cost):
        if a == nA:
            found.append((pairs, cost, tuple(cur)))
            return
        if allowed_pair(p, a, -1):
            cur[a] = -1
            rec(a + 1, used, pairs, cost)
        for t in range(nT):
            if not (used >> t) & 1 and allowed_pair(p, a, t):
                cur[a] = t
                rec(a + 1, used | (1 << t), pairs + 1, cost + int(p["cost"][a, t]))
        cur[a] = -1

    rec(0, 0, 0, 0)
    if not found:
        return None, None, []
    K = max(f[0] for f in found)
    if K < p["min_matching"]:
        return None, None, []
    at_k = sorted((c, m) for k, c, m in found if k == K)
    return K, at_k[0][0], at_k


def hungarian(cost):
    """Textbook O(n^3) shortest-augmenting-path solver on the matrix padded with one no-task column per agent.  Returns
    (K, cost) of the unconstrained problem.  Used only beyond brute force, after a CPU test has checked it against brute."""
    c = np.asarray(cost, dtype=np.int64)
    n, nT = c.shape
    if n == 0:
        return 0, 0
    big, inf = 1 << 40, 1 << 52  # no task: above any sum of real costs; no edge: above 64 no-task prices
    m = nT + n
    a = np.full((n + 1, m + 1), inf, dtype=np.int64)
    a[1:, 1:nT + 1] = np.where(c == NO_EDGE, inf, c)
    for i in range(n):
        a[i + 1, nT + 1 + i] = big
    u = np.zeros(n + 1, dtype=np.int64)
    v = np.zeros(m + 1, dtype=np.int64)
    pcol = np.zeros(m + 1, dtype=np.int64)
    way = np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        pcol[0] = i
        j0 = 0
        minv = np.full(m + 1, 1 << 62, dtype=np.int64)
        used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = pcol[j0]
            cur = a[i0] - u[i0] - v
            upd = ~used & (cur < minv)
            minv[upd] = cur[upd]
            way[upd] = j0
            cand = np.where(used, 1 << 62, minv)
            cand[0] = 1 << 62
            j1 = int(np.argmin(cand))
            delta = cand[j1]
            u[pcol[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if pcol[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            pcol[j0] = pcol[j1]
            j0 = j1
    K, total = 0, 0
    for j in range(1, nT + 1):
        if pcol[j]:
            K += 1
            total += int(c[pcol[j] - 1, j - 1])
    return K, total


def check_matching(p, status, matched, cost, task_of):
    """task_of is a valid matching that respects the constraints, with `matched` pairs summing to `cost`."""
    assert status == OK
    assert len(task_of) == p["nA"]
    got = [t for t in task_of if t >= 0]
    assert len(set(got)) == len(got), ("a task given twice", task_of)
    assert all(-1 <= t < p["nT"] for t in task_of)
    for a, t in enumerate(task_of):
        assert allowed_pair(p, a, t), ("pair not allowed", a, t)
    assert matched == len(got)
    assert cost == sum(int(p["cost"][a, t]) for a, t in enumerate(task_of) if t >= 0)
    assert matched >= p["min_matching"]


FOUR = [[90, 76, 75, 80], [35, 85, 55, 65], [125, 95, 90, 105], [45, 110, 95, 115]]  # test_next_best_assignment.py:76-93
X = NO_EDGE


def reference_cases():
    """The reference's own tests (test/test_assignment.py, test/test_next_best_assignment.py)."""
    return {
        "empty": problem(np.zeros((0, 0))),
        "1by2": problem([[2, 1]]),
        "2by1": problem([[2], [1]]),
        "2by2": problem([[90, 76], [35, 85]]),
        "4by4": problem(FOUR),
    }


def small_cases():
    """Fixed cases brute force can enumerate (also the series' fixed cases)."""
    c = dict(reference_cases())
    c["3by5_missing"] = problem([[4, X, 3, X, 9], [X, 2, X, X, 2], [7, X, X, 1, X]])
    c["5by3_missing"] = problem([[4, X, 3], [X, 2, X], [7, X, X], [X, X, 1], [9, 2, X]])
    c["agent_without_edge"] = problem([[3, 1, 2], [X, X, X], [2, 2, 9]])
    c["no_agents"] = problem(np.zeros((0, 3)))
    c["no_tasks"] = problem(np.zeros((3, 0)))
    c["ties_3by3"] = problem(np.zeros((3, 3)))
    c["max_cost_2by2"] = problem([[MAX_COST, MAX_COST], [MAX_COST, 0]])
    return c


def constraint_cases():
    """One case per mode, the mask, min_matching; then every infeasibility reason."""
    c = {}
    c["forced_pair"] = problem(FOUR, mode=[0, FREE, FREE, FREE])
    c["no_task"] = problem(FOUR, mode=[FREE, NO_TASK, FREE, FREE])
    c["some_task"] = problem([[2], [1]], mode=[SOME_TASK, FREE])
    c["mask"] = problem(FOUR, forbidden=[1 << 3, 1 << 2, 0, 0])
    c["mask_high_bits_ignored"] = problem([[2, 1]], forbidden=[(1 << 63) | (1 << 2)])
    c["min_matching_met"] = problem(FOUR, min_matching=4)
    c["forced_and_mask_and_some"] = problem(FOUR, forbidden=[0, 1 << 2, 0, 1], mode=[FREE, SOME_TASK, 1, FREE], min_matching=4)
    c["infeasible_forced_no_edge"] = problem([[X, 1], [1, 1]], mode=[0, FREE])
    c["infeasible_forced_forbidden"] = problem([[1, 1], [1, 1]], forbidden=[1, 0], mode=[0, FREE])
    c["infeasible_two_forced_to_one"] = problem([[1, 1], [1, 1]], mode=[1, 1])
    c["infeasible_some_task_gets_none"] = problem([[1, X], [1, X]], mode=[SOME_TASK, SOME_TASK])
    c["infeasible_some_task_no_tasks"] = problem(np.zeros((1, 0)), mode=[SOME_TASK])
    c["infeasible_min_matching"] = problem([[1, X], [1, X]], min_matching=2)
    c["infeasible_no_task_vs_min"] = problem(FOUR, mode=[NO_TASK, FREE, FREE, FREE], min_matching=4)
    return c


def large_cases():
    """Beyond brute force: name -> (problem, K, cost) with (K, cost) known by construction or from hungarian()."""
    rng = np.random.RandomState(7)
    c = {}
    c["8by8_zeros"] = (problem(np.zeros((8, 8))), 8, 0)
    col = rng.randint(0, MAX_COST + 1, size=(64, 1))
    c["64by1"] = (problem(col), 1, int(col.min()))
    row = rng.randint(0, MAX_COST + 1, size=(1, 64))
    c["1by64"] = (problem(row), 1, int(row.min()))
    for name, shape in (("33by31", (33, 31)), ("64by64", (64, 64))):
        m = rng.randint(0, 1000, size=shape)
        c[name] = (problem(m),) + hungarian(m)
    c["64by64_max_cost"] = (problem(np.full((64, 64), MAX_COST)), 64, 64 * MAX_COST)
    d = np.full((64, 64), X, dtype=np.int64)
    diag = rng.randint(0, MAX_COST + 1, size=64)
    d[np.arange(64), np.arange(64)] = diag
    c["64by64_diagonal"] = (problem(d), 64, int(diag.sum()))
    return c


def random_problem(rng, max_dim, constraints=True):
    nA, nT = int(rng.randint(1, max_dim + 1)), int(rng.randint(1, max_dim + 1))
    hi = 4 if rng.rand() < 0.5 else MAX_COST + 1  # {0..3}: every tie; or the full range
    cost = rng.randint(0, hi, size=(nA, nT)).astype(np.int64)
    cost[rng.rand(nA, nT) > rng.uniform(0.3, 1.0)] = NO_EDGE
    forbidden = mode = None
    mm = 0
    if constraints and rng.rand() < 0.5:
        forbidden = [int(sum(1 << t for t in range(nT) if rng.rand() < 0.15)) for _ in range(nA)]
        mode = []
        for _ in range(nA):
            r = rng.rand()
            mode.append(FREE if r < 0.6 else int(rng.randint(0, nT)) if r < 0.75 else NO_TASK if r < 0.85 else SOME_TASK)
        if rng.rand() < 0.3:
            mm = int(rng.randint(0, min(nA, nT) + 1))
    return problem(cost, forbidden, mode, mm)


def random_small(n, seed, max_dim=6, constraints=True):
    rng = np.random.RandomState(seed)
    return [random_problem(rng, max_dim, constraints) for _ in range(n)]


def random_large(n, seed):
    """20 .. 64 agents and tasks, unconstrained, some with missing edges."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        nA, nT = int(rng.randint(20, 65)), int(rng.randint(20, 65))
        cost = rng.randint(0, 50 if k % 2 else MAX_COST + 1, size=(nA, nT)).astype(np.int64)
        if k % 3 == 0:
            cost[rng.rand(nA, nT) > 0.5] = NO_EDGE
        out.append(problem(cost))
    return out


def gather_cases():
    """The gather form's inputs: a 32 x 32 and a 48 x 48 map (the two table layouts) with a walled-off 3 x 3 pocket, eight
    goals (two inside the pocket: unreachable from outside), eight starts outside and a mask of the goals each agent may
    take.  `problem` is the same problem as a matrix, built from plain BFS tables."""
    out = []
    for dim in (32, 48):
        m = hi.random_map(dim, dim, 300 + dim, density=0.1)
        wall = [[x, y] for x in range(9, 14) for y in range(9, 14) if x in (9, 13) or y in (9, 13)]
        m["obstacles"] = [o for o in m["obstacles"] if not (9 <= o[0] <= 13 and 9 <= o[1] <= 13)] + wall
        rng = np.random.RandomState(dim)
        free = [c for c in hi.free_cells(m) if not (9 <= c[0] <= 13 and 9 <= c[1] <= 13)]
        pick = rng.choice(len(free), 14, replace=False)
        goals = [(10, 10), (12, 11)] + [tuple(free[i]) for i in pick[:6]]
        starts = [tuple(free[i]) for i in pick[6:]]
        tables = [hi.bfs(m["dimx"], m["dimy"], m["obstacles"], g) for g in goals]
        allowed = [int(rng.randint(1, 256)) | 4 for _ in starts]
        cost = np.array([[NO_EDGE if not (allowed[a] >> t) & 1 else int(tables[t][s[1], s[0]]) for t in range(len(goals))]
                         for a, s in enumerate(starts)], dtype=np.int64)
        assert (cost[:, :2] == NO_EDGE).all() and (cost != NO_EDGE).any()
        out.append(dict(map=m, goals=goals, starts=starts, allowed=allowed, tables=tables, problem=problem(cost)))
    return out


def recorded_sets():
    """The problem sets whose results tests/golden/assign_task_of.json records, in a fixed order."""
    fixed = dict(small_cases())
    fixed.update(constraint_cases())
    large = large_cases()
    return {"fixed": [fixed[n] for n in sorted(fixed)], "large_fixed": [large[n][0] for n in sorted(large)],
            "random_small_seed1": random_small(1000, 1), "random_large_seed2": random_large(64, 2)}


def recorded_task_of():
    """name -> [[status, matched, cost, task_of]] as the emulator of the wave program gave them."""
    with open(os.path.join(GOLDEN, "assign_task_of.json")) as f:
        return json.load(f)
