"""Shared inputs of the wide assignment tests (up to 256 x 256): the emulator test, the golden script and the GPU test
build the same problems from here.  Problems are the dicts of tests/assignment_inputs.py; a forbidden mask is a Python int
of any width.  Oracles: ai.brute for problems embedded on scattered indices, ai.hungarian otherwise."""
import json
import os

import numpy as np

import assignment_inputs as ai

SCATTER = [0, 63, 64, 65, 127, 128, 191, 192, 255]
SHAPES = [(64, 65), (65, 64), (65, 65), (1, 256), (256, 1), (128, 129), (129, 128), (192, 193), (255, 256), (256, 256)]
GOLDEN_FILE = os.path.join(ai.GOLDEN, "assign_wide_task_of.json")


def embed(p, rng, agent_pool=SCATTER):
    """The small problem p on scattered agent and task indices, inside a problem whose other rows and columns have no
    edges; masks and forced tasks remapped.  Returns (big problem, agent indices, task indices)."""
    ag = sorted(rng.choice(agent_pool, p["nA"], replace=False).tolist())
    tk = sorted(rng.choice(SCATTER, p["nT"], replace=False).tolist())
    nA, nT = ag[-1] + 1, tk[-1] + 1
    cost = np.full((nA, nT), ai.NO_EDGE, dtype=np.int64)
    cost[np.ix_(ag, tk)] = p["cost"]
    forbidden = mode = None
    if p["forbidden"] is not None:
        forbidden = [0] * nA
        for a, f in zip(ag, p["forbidden"]):
            forbidden[a] = sum(1 << tk[t] for t in range(p["nT"]) if (f >> t) & 1)
    if p["mode"] is not None:
        mode = [ai.FREE] * nA
        for a, m in zip(ag, p["mode"]):
            mode[a] = tk[m] if m >= 0 else m
    return ai.problem(cost, forbidden, mode, p["min_matching"]), ag, tk


def embedded_small():
    """Group 2: [(small problem, big problem)] for ai.random_small(300, 3, max_dim=5), constraints included."""
    rng = np.random.RandomState(17)
    return [(p, embed(p, rng)[0]) for p in ai.random_small(300, 3, max_dim=5)]


def embedded_series():
    """Group 3: the first 30 of those problems with 4 or fewer agents, unconstrained (a series takes no constraints),
    embedded again: [(small problem, big problem, agent indices, task indices)].  A step of a series solves one child
    per agent of the big problem, so the time goes with the square of the highest agent index: every sixth problem draws
    its agents from all of SCATTER, the others from its indices up to 65; the tasks always come from all of SCATTER."""
    rng = np.random.RandomState(19)
    out = []
    for p in ai.random_small(300, 3, max_dim=5):
        if p["nA"] <= 4 and len(out) < 30:
            q = ai.problem(p["cost"])
            out.append((q,) + embed(q, rng, SCATTER if len(out) % 6 == 5 else SCATTER[:4]))
    return out


def shape_problems():
    """Group 4: name -> problem; costs 0 .. 1000, 15 % no edge."""
    rng = np.random.RandomState(23)
    out = {}
    for nA, nT in SHAPES:
        c = rng.randint(0, 1001, size=(nA, nT)).astype(np.int64)
        c[rng.rand(nA, nT) < 0.15] = ai.NO_EDGE
        out["%dx%d" % (nA, nT)] = ai.problem(c)
    return out


def max_cost_problem():
    """Group 5: 256 x 256, every cost 2^24 - 1: K = 256, cost 256 x (2^24 - 1) = 4 294 967 040."""
    return ai.problem(np.full((256, 256), ai.MAX_COST))


def constraint_problems():
    """Group 6, constraints beyond bit 63: name -> (problem, expectation), the expectation being None (infeasible) or the
    unconstrained matrix whose ai.hungarian gives (K, cost), with a (K, cost) offset for a forced pair."""
    rng = np.random.RandomState(29)
    base = rng.randint(1, 1001, size=(256, 256)).astype(np.int64)
    out = {}
    # agent 0's four cheapest tasks are forbidden to it
    c = base.copy()
    bits = [64, 127, 128, 255]
    c[0, bits] = 0
    masked = c.copy()
    masked[0, bits] = ai.NO_EDGE
    out["forbidden_64_127_128_255"] = (ai.problem(c, forbidden=[sum(1 << b for b in bits)] + [0] * 255), (masked, 0, 0))
    # agent 3 forced to task 255, an expensive pair
    c = base.copy()
    c[3, 255] = 5000
    rest = np.delete(np.delete(c, 3, axis=0), 255, axis=1)
    out["forced_255"] = (ai.problem(c, mode=[ai.FREE] * 3 + [255] + [ai.FREE] * 252), (rest, 1, 5000))
    mode = [ai.FREE] * 256
    mode[10] = mode[130] = 200
    out["infeasible_two_forced_to_200"] = (ai.problem(base, mode=mode), None)
    c = base.copy()
    c[200, :] = ai.NO_EDGE
    mode = [ai.FREE] * 256
    mode[200] = ai.SOME_TASK
    out["infeasible_agent_200_some_task_no_edge"] = (ai.problem(c, mode=mode), None)
    out["min_matching_256_met"] = (ai.problem(base, min_matching=256), (base, 0, 0))
    c = base.copy()
    c[7, :] = ai.NO_EDGE
    out["infeasible_min_matching_256_missed_by_one"] = (ai.problem(c, min_matching=256), None)
    return out


_expected = {}


def expected(name, expectation):
    """(status, K, cost) of a group-4 or group-6 problem, from ai.hungarian (computed once per process)."""
    if name not in _expected:
        if expectation is None:
            _expected[name] = (ai.INFEASIBLE, 0, 0)
        else:
            matrix, dk, dc = expectation
            K, cost = ai.hungarian(matrix)
            _expected[name] = (ai.OK, K + dk, cost + dc)
    return _expected[name]


def recorded_names():
    return sorted(shape_problems()) + sorted(constraint_problems())


def recorded_task_of():
    """name -> [status, matched, cost, task_of] as the emulator of the wide wave program gave them (both row sources)."""
    with open(GOLDEN_FILE) as f:
        return json.load(f)
