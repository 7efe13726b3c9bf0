"""Min-cost task assignment and its next-best series on the MI355X (mrp_ll_assign_batch, mrp_ll_assign_series_*):
the inputs and oracles of the emulator test (tests/assignment_inputs.py) through the C ABI — one launch per batch and
per series step, results independent of a problem's place in the batch, the gather form over device-resident heuristic
tables against the same problem as a matrix, the error codes, and the two CLI front-ends.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import assignment_inputs as ai
from libmultirobotplanning_amd import yaml_subset

pytestmark = pytest.mark.gpu

E_INVALID, E_BUSY = -1, -4


@pytest.fixture(scope="module")
def eng():
    from libmultirobotplanning_amd import ll
    e = ll.LowLevelEngine(n_tickets=1, slots=16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch():
    """The fixed cases and the random sets of the CPU test, as one batch: [(name, problem, expectation)] where the
    expectation is ("brute",) or ("known", K, cost)."""
    rows = []
    small = dict(ai.small_cases())
    small.update(ai.constraint_cases())
    rows += [(n, small[n], ("brute",)) for n in sorted(small)]
    large = ai.large_cases()
    rows += [(n, large[n][0], ("known",) + large[n][1:]) for n in sorted(large)]
    rows += [("small%d" % k, p, ("brute",)) for k, p in enumerate(ai.random_small(1000, 1))]
    rows += [("large%d" % k, p, ("known",) + ai.hungarian(p["cost"])) for k, p in enumerate(ai.random_large(64, 2))]
    return rows


def _as_tuple(r):
    return r.status, r.matched, r.cost, r.task_of


def _check(p, r, expect, what):
    if expect[0] == "known":
        assert _as_tuple(r)[:3] == (ai.OK,) + tuple(expect[1:]), (what, _as_tuple(r)[:3], expect)
        ai.check_matching(p, *_as_tuple(r))
        return
    K, best, _ = ai.brute(p)
    if K is None:
        assert _as_tuple(r) == (ai.INFEASIBLE, 0, 0, [-1] * p["nA"]), what
    else:
        assert _as_tuple(r)[:3] == (ai.OK, K, best), (what, _as_tuple(r), K, best)
        ai.check_matching(p, *_as_tuple(r))


def test_batch_in_one_launch_equals_oracles(eng, batch):
    before = eng.stats()["launches"]
    res = eng.assign_batch([p for _, p, _ in batch])
    assert eng.stats()["launches"] == before + 1
    assert len(res) == len(batch)
    for (name, p, expect), r in zip(batch, res):
        _check(p, r, expect, name)
    by = {name: r for (name, _, _), r in zip(batch, res)}
    assert by["2by1"].task_of == [-1, 0] and by["2by1"].cost == 1
    assert by["4by4"].task_of == [3, 2, 1, 0] and by["4by4"].cost == 275
    assert by["64by64_max_cost"].cost == 64 * 16777215
    assert eng.assign_batch([]) == [] and eng.stats()["launches"] == before + 1  # n == 0: no launch


def test_result_does_not_depend_on_position(eng, batch):
    probs = [p for _, p, _ in batch]
    fwd = eng.assign_batch(probs)
    rev = eng.assign_batch(probs[::-1])[::-1]
    assert [_as_tuple(r) for r in fwd] == [_as_tuple(r) for r in rev]
    for k in (0, 7, len(probs) - 1, len(probs) - 40):
        assert _as_tuple(eng.assign_batch([probs[k]])[0]) == _as_tuple(fwd[k]), k


def test_task_of_equals_the_emulator_s(eng):
    """Determinism: the device's matchings equal, entry for entry, the ones the CPU emulator of the same wave program
    recorded in tests/golden/assign_task_of.json (tests/test_assign_emu_cpu.py holds the emulator to that file)."""
    want, sets = ai.recorded_task_of(), ai.recorded_sets()
    assert sorted(want) == sorted(sets)
    for name in sorted(sets):
        got = eng.assign_batch(sets[name])
        assert [list(_as_tuple(r)) for r in got] == want[name], name


def test_gather_form_equals_matrix_from_lookup(eng):
    """cost(a, t) straight from the device's tables (32 x 32 and 48 x 48: both table layouts), two goals in a walled-off
    pocket (unreachable = no edge), some pairs masked out — against the same problem given as a matrix built from
    heuristic_lookup, and against the matrix built from plain BFS tables."""
    for g in ai.gather_cases():
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
        assert np.array_equal(cost, g["problem"]["cost"])
        gather = dict(heuristic_ids=hids, starts=[list(s) for s in g["starts"]], allowed=g["allowed"])
        got, want = eng.assign_batch([gather, ai.problem(cost)])
        assert _as_tuple(got) == _as_tuple(want)
        assert _as_tuple(got)[:3] == (ai.OK,) + ai.hungarian(cost)
        ai.check_matching(g["problem"], *_as_tuple(got))
        # constrained, as a series' child is: a forced pair, a forbidden pair, a required cardinality
        with_task = [a for a in range(nA) if got.task_of[a] >= 0]
        assert len(with_task) >= 2
        forb = [0] * nA
        forb[with_task[1]] = 1 << got.task_of[with_task[1]]
        mode = [ai.FREE] * nA
        mode[with_task[0]] = got.task_of[with_task[0]]
        con = dict(forbidden=forb, mode=mode, min_matching=got.matched)
        a, b = eng.assign_batch([dict(gather, **con), ai.problem(cost, **con)])
        assert _as_tuple(a) == _as_tuple(b)
        # a gather-form series keeps reading the tables
        s_g, s_m = eng.assign_series([gather, dict(cost=cost)])
        for _ in range(5):
            x, y = eng.assign_series_next([s_g, s_m])
            assert _as_tuple(x) == _as_tuple(y)
        assert x.status == ai.OK  # (far more than five matchings of that cardinality)
        s_g.close()
        s_m.close()


def test_series_many_together_equal_brute(eng):
    from libmultirobotplanning_amd.ll import AssignmentSeries
    probs = ai.random_small(64, 4, max_dim=5, constraints=False)
    series = eng.assign_series(probs)
    got = [[] for _ in probs]
    alive = list(range(len(probs)))
    steps = 0
    while alive:
        before = eng.stats()["launches"]
        res = AssignmentSeries.next_many([series[k] for k in alive])
        # ONE launch per step, however many series are alive (none once no popped node has a child)
        launches = eng.stats()["launches"] - before
        assert launches == 1 if steps == 0 else launches <= 1
        steps += 1
        still = []
        for k, r in zip(alive, res):
            if r.status == ai.OK:
                got[k].append((r.cost, tuple(r.task_of)))
                still.append(k)
            else:
                assert (r.status, r.matched) == (ai.INFEASIBLE, 0)
        alive = still
        assert steps < 200
    for k, p in enumerate(probs):
        K, _, at_k = ai.brute(p)
        assert [c for c, _ in got[k]] == [c for c, _ in at_k], k
        assert sorted(got[k]) == at_k, k
    for s in series[:3]:  # exhausted stays exhausted
        r = s.next()
        assert (r.status, r.matched) == (ai.INFEASIBLE, 0)
    for s in series:
        s.close()


def test_series_reference_cases(eng):
    cases = ai.reference_cases()
    two = eng.assign_series([cases["2by1"]])[0]
    assert [(r.cost, r.task_of) for r in (two.next(), two.next())] == [(1, [-1, 0]), (2, [0, -1])]
    assert two.next().status == ai.INFEASIBLE and two.next().status == ai.INFEASIBLE
    two.close()
    four = eng.assign_series([cases["4by4"]])[0]
    sols = []
    while True:
        r = four.next()
        if r.status != ai.OK:
            break
        sols.append((r.cost, tuple(r.task_of)))
    four.close()
    _, _, at_k = ai.brute(cases["4by4"])
    assert len(sols) == 24 and sols[0] == (275, (3, 2, 1, 0)) and sols[-1] == (400, (2, 1, 0, 3))
    assert [c for c, _ in sols] == [c for c, _ in at_k] and sorted(sols) == at_k


def test_error_codes(eng):
    from libmultirobotplanning_amd import ll
    lib, h = eng._lib, eng._h
    good = ai.reference_cases()["2by2"]
    carr, keep, dims = eng._marshal_assign([good])
    cres, task_of = eng._assign_results(dims)
    assert lib.mrp_ll_assign_batch(None, 1, carr, cres) == E_INVALID
    assert lib.mrp_ll_assign_batch(h, 1, None, cres) == E_INVALID
    assert lib.mrp_ll_assign_batch(h, 1, carr, None) == E_INVALID
    hs = (ctypes.c_void_p * 1)()
    assert lib.mrp_ll_assign_series_create(h, 1, carr, None) == E_INVALID
    assert lib.mrp_ll_assign_series_next(h, 1, None, cres) == E_INVALID
    constrained = dict(good, mode=[ai.FREE, ai.FREE])
    c2, keep2, _ = eng._marshal_assign([constrained])
    assert lib.mrp_ll_assign_series_create(h, 1, c2, hs) == E_INVALID and not hs[0]
    # BAD_JOB: the problem is not run, its neighbours are unaffected
    bad = [ai.problem(np.zeros((65, 1))), ai.problem(np.zeros((1, 65))), ai.problem([[ai.MAX_COST + 1]]), ai.problem([[-1]]),
           ai.problem([[1, 2]], mode=[2]), ai.problem([[1, 2]], mode=[-4]), ai.problem([[1]], min_matching=65),
           dict(heuristic_ids=[10 ** 6], starts=[[0, 0]])]
    mixed = [good]
    for b in bad:
        mixed += [b, good]
    res = eng.assign_batch(mixed)
    assert [r.status for r in res] == [ai.OK] + [ai.BAD_JOB, ai.OK] * len(bad)
    assert all((r.cost, r.task_of) == (111, [1, 0]) for r in res[::2])
    assert all((r.matched, r.cost) == (0, 0) for r in res[1::2])
    # E_BUSY inside a session
    series = eng.assign_series([good])[0]
    eng.session_begin(16)
    try:
        assert lib.mrp_ll_assign_batch(h, 1, carr, cres) == E_BUSY
        assert lib.mrp_ll_assign_series_create(h, 1, carr, hs) == E_BUSY
        hs1 = (ctypes.c_void_p * 1)(series._h)
        assert lib.mrp_ll_assign_series_next(h, 1, hs1, cres) == E_BUSY
    finally:
        eng.session_end()
    assert series.next().cost == 111  # the refused step took nothing from the series
    series.close()
    assert ll.BAD_JOB == ai.BAD_JOB


def _write_pairs(path, p, sep="->"):
    with open(path, "w") as f:
        for a in range(p["nA"]):
            for t in range(p["nT"]):
                if p["cost"][a, t] != ai.NO_EDGE:
                    f.write("a%d%st%d:%d\n" % (a, sep, t, p["cost"][a, t]))


def test_cli_front_ends(tmp_path, capsys):
    from libmultirobotplanning_amd import cli
    cases = ai.reference_cases()
    for name in ("4by4", "2by2", "2by1", "1by2", "empty"):
        p = cases[name]
        inp, out = str(tmp_path / (name + ".txt")), str(tmp_path / (name + ".yaml"))
        _write_pairs(inp, p, " -> " if name == "2by1" else "->")
        K, best, at_k = ai.brute(p)
        assert cli.main(["assignment", "-i", inp, "-o", out]) == 0
        doc = yaml_subset.load(out)
        assert doc["cost"] == best
        want = {"a%d" % a: "t%d" % t for a, t in enumerate(at_k[0][1]) if t >= 0}
        assert (doc["assignment"] or {}) == want
        assert cli.main(["next_best_assignment", "-i", inp, "-o", out]) == 0
        sols = yaml_subset.load(out)["solutions"] or []
        assert len(sols) == (len(at_k) if K else 0)
        if K:
            got = [(s["cost"], tuple(sorted(s["assignment"].items()))) for s in sols]
            exp = [(c, tuple(sorted(("a%d" % a, "t%d" % t) for a, t in enumerate(m) if t >= 0))) for c, m in at_k]
            assert [c for c, _ in got] == [c for c, _ in exp] and sorted(got) == sorted(exp)
            assert got[0] == exp[0] and got[-1] == exp[-1]
    with open(tmp_path / "odd.txt", "w") as f:
        f.write("a0->t0:2\nnot a pair\na1->t0:1\n")
    capsys.readouterr()
    assert cli.main(["assignment", "-i", str(tmp_path / "odd.txt"), "-o", str(tmp_path / "odd.yaml")]) == 0
    assert "Couldn't match line \"not a pair\"" in capsys.readouterr().err
    assert yaml_subset.load(str(tmp_path / "odd.yaml")) == {"cost": 1, "assignment": {"a1": "t0"}}
    with open(tmp_path / "wide.txt", "w") as f:
        for a in range(65):
            f.write("a%d->t0:1\n" % a)
    assert cli.main(["assignment", "-i", str(tmp_path / "wide.txt"), "-o", str(tmp_path / "wide.yaml")]) != 0
    assert "at most 64" in capsys.readouterr().err
