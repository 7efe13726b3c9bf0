"""The wide assignment calls on the MI355X (mrp_ll_assign_batch_w, mrp_ll_assign_series_create_w: up to 256 agents x 256
tasks): the inputs, oracles and recorded matchings of the emulator test (tests/assignment_wide_inputs.py,
tests/golden/assign_wide_task_of.json) through the C ABI — one launch per batch, results independent of a problem's place
and of where its cost rows live (LDS, or device memory: a fresh process with MRP_LL_ASSIGN_LDS_BYTES=0 sends every problem
there), the narrow golden matchings through the wide call, the gather form against the same problem as a matrix, narrow
and wide series advancing together, the error codes and the --wide flag of the two CLI front-ends.  All comparisons are
exact."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import assignment_inputs as ai
import assignment_wide_inputs as wi
import heuristic_inputs as hi
from libmultirobotplanning_amd import yaml_subset

pytestmark = pytest.mark.gpu

E_INVALID, E_BUSY = -1, -4
TESTS = os.path.dirname(os.path.abspath(__file__))


def _as_tuple(r):
    return r.status, r.matched, r.cost, r.task_of


def batch_rows():
    """Groups 2, 4, 5 and 6 of the emulator test as one batch: [(name, problem, expectation)], the expectation being
    ("brute", small problem), ("hungarian", expectation of wi.expected) or ("known", K, cost)."""
    rows = [("embedded%d" % k, big, ("brute", small)) for k, (small, big) in enumerate(wi.embedded_small())]
    rows += [(n, p, ("hungarian", (p["cost"], 0, 0))) for n, p in sorted(wi.shape_problems().items())]
    rows.append(("256x256_max_cost", wi.max_cost_problem(), ("known", 256, 256 * ai.MAX_COST)))
    rows += [(n, p, ("hungarian", e)) for n, (p, e) in sorted(wi.constraint_problems().items())]
    return rows


def gather_cases():
    """A 32 x 32 map with 70 goals and 70 agents (two mask words) and a 48 x 48 map with 130 goals and 100 agents (three;
    more than the default budget's LDS rows), each with a walled-off 3 x 3 pocket that holds two goals (unreachable from
    outside: no edge) and an `allowed` mask that takes about a fifth of the pairs out."""
    out = []
    for dim, n_goals, n_agents in ((32, 70, 70), (48, 130, 100)):
        m = hi.random_map(dim, dim, 500 + dim, density=0.1)
        wall = [[x, y] for x in range(9, 14) for y in range(9, 14) if x in (9, 13) or y in (9, 13)]
        m["obstacles"] = [o for o in m["obstacles"] if not (9 <= o[0] <= 13 and 9 <= o[1] <= 13)] + wall
        rng = np.random.RandomState(dim)
        free = [c for c in hi.free_cells(m) if not (9 <= c[0] <= 13 and 9 <= c[1] <= 13)]
        pick = rng.choice(len(free), n_goals - 2 + n_agents, replace=False)
        goals = [tuple(free[i]) for i in pick[:n_goals - 2]]
        goals[5:5] = [(10, 10)]      # the pocket's goals at indices 5 and 66: one in each of the first two mask words
        goals[66:66] = [(12, 11)]
        starts = [tuple(free[i]) for i in pick[n_goals - 2:]]
        allowed = [sum(1 << t for t in range(n_goals) if rng.rand() < 0.8) | 1 << (n_goals - 1) for _ in starts]
        out.append(dict(map=m, goals=goals, starts=starts, allowed=allowed))
    return out


def solve_everything(eng):
    """What both processes compute: the batch's results and, per gather case, (gather result, matrix result, matrix)."""
    res = {"batch": [list(_as_tuple(r)) for r in eng.assign_batch([p for _, p, _ in batch_rows()], wide=True)], "gather": []}
    for g in gather_cases():
        m = g["map"]
        mid = eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        hids = eng.compute_heuristics([mid] * len(g["goals"]), [list(x) for x in g["goals"]])
        nA, nT = len(g["starts"]), len(hids)
        looked = eng.heuristic_lookup([h for _ in range(nA) for h in hids], [list(s) for s in g["starts"] for _ in hids])
        cost = looked.astype(np.int64).reshape(nA, nT)
        for a in range(nA):
            for t in range(nT):
                if not (g["allowed"][a] >> t) & 1:
                    cost[a, t] = ai.NO_EDGE
        gather = dict(heuristic_ids=hids, starts=[list(s) for s in g["starts"]], allowed=g["allowed"])
        got, want = eng.assign_batch([gather, ai.problem(cost)], wide=True)
        res["gather"].append([list(_as_tuple(got)), list(_as_tuple(want)), cost.tolist()])
    return res


def child_main():
    """The fresh process of test_memory_rows_give_the_same_answers: everything again, as JSON on stdout."""
    from libmultirobotplanning_amd import ll
    e = ll.LowLevelEngine(n_tickets=1, slots=16)
    try:
        print("RESULTS " + json.dumps(solve_everything(e)))
    finally:
        e.close()


@pytest.fixture(scope="module")
def eng():
    from libmultirobotplanning_amd import ll
    e = ll.LowLevelEngine(n_tickets=1, slots=16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch():
    return batch_rows()


@pytest.fixture(scope="module")
def solved(eng):
    before = eng.stats()["launches"]
    res = solve_everything(eng)
    return res, eng.stats()["launches"] - before


def test_batch_in_one_launch_equals_oracles_and_recorded_matchings(eng, batch):
    before = eng.stats()["launches"]
    res = eng.assign_batch([p for _, p, _ in batch], wide=True)
    assert eng.stats()["launches"] == before + 1
    assert len(res) == len(batch)
    golden = wi.recorded_task_of()
    seen = 0
    for (name, p, expect), r in zip(batch, res):
        if expect[0] == "brute":
            K, best, _ = ai.brute(expect[1])
            want = (ai.INFEASIBLE, 0, 0) if K is None else (ai.OK, K, best)
        elif expect[0] == "hungarian":
            want = wi.expected(name, expect[1])
        else:
            want = (ai.OK,) + tuple(expect[1:])
        assert _as_tuple(r)[:3] == want, (name, _as_tuple(r)[:3], want)
        if want[0] == ai.OK:
            ai.check_matching(p, *_as_tuple(r))
        else:
            assert r.task_of == [-1] * p["nA"], name
        if name in golden:
            assert list(_as_tuple(r)) == golden[name], name
            seen += 1
    assert seen == len(golden) == len(wi.recorded_names())
    assert eng.assign_batch([], wide=True) == [] and eng.stats()["launches"] == before + 1  # n == 0: no launch


def test_result_does_not_depend_on_position(eng, batch, solved):
    probs = [p for _, p, _ in batch]
    fwd = [tuple(r) for r in solved[0]["batch"]]
    rev = eng.assign_batch(probs[::-1], wide=True)[::-1]
    assert [_as_tuple(r) for r in rev] == fwd
    for k in (0, 7, 299, 300, len(probs) - 8, len(probs) - 6, len(probs) - 1):
        assert _as_tuple(eng.assign_batch([probs[k]], wide=True)[0]) == fwd[k], k


def test_memory_rows_give_the_same_answers(solved):
    """The same calls in a fresh process whose engine reads MRP_LL_ASSIGN_LDS_BYTES=0: every problem with agents takes its
    cost rows from device memory (the gather form through its scratch region).  The answers are identical."""
    env = dict(os.environ, MRP_LL_ASSIGN_LDS_BYTES="0",
               PYTHONPATH=os.pathsep.join([TESTS, os.path.dirname(TESTS)] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    run = subprocess.run([sys.executable, "-s", "-c", "import test_assign_wide_gpu as t; t.child_main()"], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]
    line = [l for l in run.stdout.splitlines() if l.startswith("RESULTS ")]
    assert len(line) == 1
    assert json.loads(line[0][len("RESULTS "):]) == solved[0]


def test_narrow_sets_through_the_wide_call_equal_the_recorded_task_of(eng):
    want, sets = ai.recorded_task_of(), ai.recorded_sets()
    for name in sorted(sets):
        got = eng.assign_batch(sets[name], wide=True)
        assert [list(_as_tuple(r)) for r in got] == want[name], name


def test_gather_form_equals_matrix_from_lookup(solved):
    cases = gather_cases()
    assert len(solved[0]["gather"]) == len(cases) == 2
    for g, (got, want, cost) in zip(cases, solved[0]["gather"]):
        cost = np.array(cost, dtype=np.int64)
        assert cost.shape == (len(g["starts"]), len(g["goals"]))
        assert (cost[:, 5] == ai.NO_EDGE).all() and (cost[:, 66] == ai.NO_EDGE).all() and (cost != ai.NO_EDGE).any()
        assert got == want
        assert tuple(got[:3]) == (ai.OK,) + ai.hungarian(cost)
        ai.check_matching(ai.problem(cost), *got)


def test_narrow_and_wide_series_advance_together(eng):
    rng = np.random.RandomState(41)
    c = rng.randint(0, 1001, size=(70, 70)).astype(np.int64)
    c[rng.rand(70, 70) < 0.15] = ai.NO_EDGE
    four = ai.reference_cases()["4by4"]
    wide = eng.assign_series([ai.problem(c)], wide=True)[0]
    narrow = eng.assign_series([four])[0]
    K, best = ai.hungarian(c)
    _, _, at_k = ai.brute(four)
    wide_sols, narrow_sols = [], []
    for step in range(26):
        before = eng.stats()["launches"]
        w, n = eng.assign_series_next([wide, narrow])
        launches = eng.stats()["launches"] - before
        assert launches == 2 if step == 0 else launches <= 2, step
        if step < 20:
            assert (w.status, w.matched) == (ai.OK, K)
            ai.check_matching(ai.problem(c), *_as_tuple(w))
            wide_sols.append((w.cost, tuple(w.task_of)))
        if n.status == ai.OK:
            narrow_sols.append((n.cost, tuple(n.task_of)))
        else:
            assert step >= 24 and (n.status, n.matched) == (ai.INFEASIBLE, 0)
    assert wide_sols[0][0] == best
    assert [s[0] for s in wide_sols] == sorted(s[0] for s in wide_sols) and len(set(wide_sols)) == 20
    assert [s[0] for s in narrow_sols] == [s[0] for s in at_k] and sorted(narrow_sols) == at_k
    before = eng.stats()["launches"]
    assert wide.next().status == ai.OK and eng.stats()["launches"] == before + 1  # series of one kind: one launch
    wide.close()
    narrow.close()


def test_error_codes(eng):
    from libmultirobotplanning_amd import ll
    lib, h = eng._lib, eng._h
    good = ai.reference_cases()["2by2"]
    carr, keep, dims = eng._marshal_assign([good], wide=True)
    cres, task_of = eng._assign_results(dims)
    assert lib.mrp_ll_assign_batch_w(None, 1, carr, cres) == E_INVALID
    assert lib.mrp_ll_assign_batch_w(h, 1, None, cres) == E_INVALID
    assert lib.mrp_ll_assign_batch_w(h, 1, carr, None) == E_INVALID
    hs = (ctypes.c_void_p * 1)()
    assert lib.mrp_ll_assign_series_create_w(h, 1, carr, None) == E_INVALID
    assert lib.mrp_ll_assign_series_create_w(None, 1, carr, hs) == E_INVALID
    constrained = dict(good, mode=[ai.FREE, ai.FREE])
    c2, keep2, _ = eng._marshal_assign([constrained], wide=True)
    assert lib.mrp_ll_assign_series_create_w(h, 1, c2, hs) == E_INVALID and not hs[0]
    # BAD_JOB: the problem is not run, its neighbours are unaffected
    masked65 = ai.problem(np.zeros((1, 65)), forbidden=[1 << 64])
    bad = [ai.problem(np.zeros((257, 1))), ai.problem(np.zeros((1, 257))), dict(good, mask_words=0), dict(good, mask_words=5),
           dict(masked65, mask_words=1), ai.problem([[1]], min_matching=257), ai.problem([[ai.MAX_COST + 1]]),
           ai.problem([[1, 2]], mode=[2])]
    mixed = [good]
    for b in bad:
        mixed += [b, good]
    res = eng.assign_batch(mixed, wide=True)
    assert [r.status for r in res] == [ai.OK] + [ai.BAD_JOB, ai.OK] * len(bad)
    assert all((r.cost, r.task_of) == (111, [1, 0]) for r in res[::2])
    assert all((r.matched, r.cost) == (0, 0) for r in res[1::2])
    assert eng.assign_batch([masked65], wide=True)[0].status == ai.OK  # (two mask words: sound, task 64 forbidden)
    assert eng.assign_batch([ai.problem(np.zeros((65, 1)))])[0].status == ai.BAD_JOB  # the narrow call keeps its limit
    with pytest.raises(RuntimeError):
        eng.assign_series([ai.problem(np.zeros((257, 1)))], wide=True)
    # E_BUSY inside a session
    series = eng.assign_series([good], wide=True)[0]
    eng.session_begin(16)
    try:
        assert lib.mrp_ll_assign_batch_w(h, 1, carr, cres) == E_BUSY
        assert lib.mrp_ll_assign_series_create_w(h, 1, carr, hs) == E_BUSY
        hs1 = (ctypes.c_void_p * 1)(series._h)
        assert lib.mrp_ll_assign_series_next(h, 1, hs1, cres) == E_BUSY
    finally:
        eng.session_end()
    assert series.next().cost == 111  # the refused step took nothing from the series
    series.close()
    assert ll.BAD_JOB == ai.BAD_JOB


def test_cli_wide_flag(tmp_path, capsys):
    from libmultirobotplanning_amd import cli
    with open(tmp_path / "wide.txt", "w") as f:  # the file the narrow command refuses
        for a in range(65):
            f.write("a%d->t0:1\n" % a)
    assert cli.main(["assignment", "--wide", "-i", str(tmp_path / "wide.txt"), "-o", str(tmp_path / "wide.yaml")]) == 0
    doc = yaml_subset.load(str(tmp_path / "wide.yaml"))
    assert doc["cost"] == 1 and list(doc["assignment"].values()) == ["t0"]
    capsys.readouterr()
    assert cli.main(["assignment", "-i", str(tmp_path / "wide.txt"), "-o", str(tmp_path / "narrow.yaml")]) != 0
    assert "at most 64" in capsys.readouterr().err
    rng = np.random.RandomState(43)
    c = rng.randint(0, 1001, size=(100, 100)).astype(np.int64)
    with open(tmp_path / "hundred.txt", "w") as f:
        for a in range(100):
            for t in range(100):
                f.write("a%d -> t%d : %d\n" % (a, t, c[a, t]))
    assert cli.main(["assignment", "--wide", "-i", str(tmp_path / "hundred.txt"), "-o", str(tmp_path / "hundred.yaml")]) == 0
    doc = yaml_subset.load(str(tmp_path / "hundred.yaml"))
    K, best = ai.hungarian(c)
    assert doc["cost"] == best and len(doc["assignment"]) == K == 100
    pairs = {int(a[1:]): int(t[1:]) for a, t in doc["assignment"].items()}
    assert len(set(pairs.values())) == 100 and sum(int(c[a, t]) for a, t in pairs.items()) == best
    with open(tmp_path / "two.txt", "w") as f:  # next_best_assignment --wide: 66 agents, two of them with an edge
        for a in range(66):
            f.write("a%d->t%d:%d\n" % (a, 0 if a < 64 else 1, 100 - a))
    assert cli.main(["next_best_assignment", "--wide", "-i", str(tmp_path / "two.txt"), "-o", str(tmp_path / "two.yaml")]) == 0
    sols = yaml_subset.load(str(tmp_path / "two.yaml"))["solutions"]
    assert len(sols) == 64 * 2 and sols[0] == {"cost": 37 + 35, "assignment": {"a63": "t0", "a65": "t1"}}
    assert [s["cost"] for s in sols] == sorted(s["cost"] for s in sols)
    with open(tmp_path / "toowide.txt", "w") as f:
        for a in range(257):
            f.write("a%d->t0:1\n" % a)
    capsys.readouterr()
    assert cli.main(["assignment", "--wide", "-i", str(tmp_path / "toowide.txt"), "-o", str(tmp_path / "toowide.yaml")]) != 0
    assert "at most 256" in capsys.readouterr().err
