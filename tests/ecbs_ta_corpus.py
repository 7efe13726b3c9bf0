"""The synthetic corpus of MRP_LL_ASTAR_EPS_TA searches (tests/test_ecbs_ta_parity_gpu.py), generated on the CPU with the
checker (tests/ecbs_ta_checker.py), fixed seeds.

Ten agents (eight on the 8 x 8 maps) are planned in turn against each other's current paths, round after round (ROUNDS: the
five kinds once, then the kinds 2 and 3 three more times with other constraint times):
  round 0  no constraints
  round 1  vertex and edge constraints along the agent's previous path
  round 2  a constraint on the goal cell 5 - 140 steps out (the agent waits at the goal for free, or comes back)
  round 3  agents WITHOUT a task that carry a late constraint on their start cell
  round 4  random constraint sets, more than 64 vertex and more than 64 edge constraints in many of them; expansion caps
Searches in which the checker counts a decrease-key event (a_star_epsilon.hpp:254-269 taken) are rare — about one in a
hundred, from the rounds where free Waits make g differ from time — so every one of them is kept, plus a fixed-stride sample
of the rest.  Four single cases close the corpus: a focal context of 136 agents, and three searches on a 48 x 48 map."""
import numpy as np

ROUNDS = (0, 1, 2, 3, 4, 2, 3, 2, 3, 2, 3)  # the rounds with free Waits come back, with other constraint times
WS = (1.3, 2.0, 1.3, 1.0, 1.3, 2.0, 2.0)  # w of a (map, round): mostly the values at which decrease-key occurs


def _case(checker, m, start, goal, vc, ec, w, agent, ctx, cap):
    o = checker.ll_search(m, start, goal, vc, ec, w=w, agent_idx=agent, ctx_paths=ctx, cap_expansions=cap)
    return dict(map=m, start=start, goal=goal, vc=vc, ec=ec, w=w, agent=agent, ctx=[list(p) for p in ctx], cap=cap, oracle=o)


def _rounds(checker, rng, m, starts, goals, salt, out):
    n = len(starts)
    d = m["dimx"]
    cur = [[] for _ in range(n)]
    for step, rnd in enumerate(ROUNDS):
        w = WS[(salt + step) % len(WS)]
        for a in range(n):
            s, g = starts[a], goals[a]
            vc, ec, cap = [], [], -1
            prev = cur[a]
            if rnd == 1 and len(prev) > 2:
                for _ in range(int(rng.integers(1, 5))):
                    t = int(rng.integers(1, len(prev)))
                    vc.append([t, prev[t][0], prev[t][1]])
                t = int(rng.integers(0, len(prev) - 1))
                ec.append([t, prev[t][0], prev[t][1], prev[t + 1][0], prev[t + 1][1]])
            elif rnd == 2:
                vc.append([int(rng.integers(5, 141)), g[0], g[1]])
                if len(prev) > 2:
                    t = int(rng.integers(1, len(prev)))
                    vc.append([t, prev[t][0], prev[t][1]])
            elif rnd == 3:
                g = None
                vc.append([int(rng.integers(20, 111)), s[0], s[1]])
                vc.append([int(rng.integers(1, 20)), int(rng.integers(0, d)), int(rng.integers(0, d))])
            elif rnd == 4:
                many = a % 2 == 0
                vc = [[int(rng.integers(1, 14)), int(rng.integers(0, d)), int(rng.integers(0, d))]
                      for _ in range(int(rng.integers(65, 91)) if many else int(rng.integers(0, 30)))]
                for _ in range(int(rng.integers(65, 91)) if many else int(rng.integers(0, 30))):
                    x, y = int(rng.integers(0, d)), int(rng.integers(0, d))
                    dx, dy = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)][int(rng.integers(0, 5))]
                    ec.append([int(rng.integers(0, 14)), x, y, x + dx, y + dy])
                vc = [v for v in vc if v[1:] != s]  # (a constraint on the start state itself never matters)
                cap = int(rng.choice([-1, -1, 25, 400]))
            c = _case(checker, m, s, g, vc, ec, w, a, cur, cap)
            c["round"] = rnd
            out.append(c)
            if c["oracle"]["rc"] == 0 and c["oracle"]["success"]:
                cur[a] = [st[1:] for st in c["oracle"]["states"]]


def generate(checker, bench_instances, n_maps32=40, n_maps8=5):
    """Returns (corpus, generated): the kept cases (generation order: every decrease-key search and every seventh of the
    others, then the four single cases) and the number of searches generated."""
    rng = np.random.default_rng(20240607)
    allc = []
    for k in range(n_maps32):
        inst = bench_instances["map_32by32_obst204_agents10_ex%d" % k]
        m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
        _rounds(checker, rng, m, inst["starts"], inst["goals"], k, allc)
    for k in range(n_maps8):
        inst = bench_instances["map_8by8_obst12_agents8_ex%d" % k]
        m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
        _rounds(checker, rng, m, inst["starts"], inst["goals"], k, allc)
    corpus = [c for i, c in enumerate(allc) if c["oracle"]["decrease_keys"] > 0 or i % 7 == 0]
    # ---- a focal context of 136 agents (beyond the two 64-lane row loads): random walks of 1 - 60 states
    inst = bench_instances["map_32by32_obst204_agents10_ex1"]
    m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
    ctx = []
    for a in range(136):
        x, y = int(rng.integers(0, 32)), int(rng.integers(0, 32))
        p = [[x, y]]
        for _ in range(int(rng.integers(0, 60))):
            dx, dy = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)][int(rng.integers(0, 5))]
            x, y = min(max(x + dx, 0), 31), min(max(y + dy, 0), 31)
            p.append([x, y])
        ctx.append(p if a % 9 else [])
    g = inst["goals"][3]
    corpus.append(_case(checker, m, inst["starts"][3], g, [[30, g[0], g[1]]], [], 1.3, 131, ctx, -1))
    # ---- a 48 x 48 map ([dimy][dimx] heuristic table): three agents in turn, the last with a late goal constraint
    obst = sorted({(int(rng.integers(0, 48)), int(rng.integers(0, 48))) for _ in range(420)})
    m48 = dict(dimx=48, dimy=48, obstacles=[list(o) for o in obst])
    free = _component(48, 48, set(obst))
    pick = [free[int(i)] for i in rng.choice(len(free), size=6, replace=False)]
    cur = [[], [], []]
    for a in range(3):
        s, g = list(pick[2 * a]), list(pick[2 * a + 1])
        c = _case(checker, m48, s, g, [[70, g[0], g[1]]] if a == 2 else [], [], 1.3, a, cur, -1)
        corpus.append(c)
        if c["oracle"]["success"]:
            cur[a] = [st[1:] for st in c["oracle"]["states"]]
    return corpus, len(allc) + 4


def _component(dimx, dimy, obst):
    """Cells of the largest 4-connected free component (the reference never returns from a search for an unreachable goal)."""
    seen, best = set(), []
    for y0 in range(dimy):
        for x0 in range(dimx):
            if (x0, y0) in obst or (x0, y0) in seen:
                continue
            comp, stack = [], [(x0, y0)]
            seen.add((x0, y0))
            while stack:
                x, y = stack.pop()
                comp.append((x, y))
                for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                    nx, ny = x + dx, y + dy
                    if 0 <= nx < dimx and 0 <= ny < dimy and (nx, ny) not in obst and (nx, ny) not in seen:
                        seen.add((nx, ny))
                        stack.append((nx, ny))
            if len(comp) > len(best):
                best = comp
    return sorted(best)


def bfs_table(dimx, dimy, obstacles, goal):
    """shortest_path_heuristic.hpp for one goal: dist[dimy][dimx], INT32_MAX = unreachable."""
    from collections import deque
    obst = {(o[0], o[1]) for o in obstacles}
    big = 2 ** 31 - 1
    dist = [[big] * dimx for _ in range(dimy)]
    if tuple(goal) in obst:
        return dist
    dist[goal[1]][goal[0]] = 0
    q = deque([tuple(goal)])
    while q:
        x, y = q.popleft()
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            nx, ny = x + dx, y + dy
            if 0 <= nx < dimx and 0 <= ny < dimy and (nx, ny) not in obst and dist[ny][nx] == big:
                dist[ny][nx] = dist[y][x] + 1
                q.append((nx, ny))
    return dist
