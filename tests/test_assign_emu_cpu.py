"""The assignment wave program (libmultirobotplanning_amd/csrc/assign_wave.h — the source the gfx950 kernel compiles) on
the CPU: tests/support/emu_assign.cpp builds it against the 64-lane lockstep interpretation of its wave vocabulary, behind
the engine's own packer (host/assign_pack.h) and next-best series (host/assign_series.h), as a program of its own under
-fsanitize=address,undefined.  Results must equal the independent oracles of tests/assignment_inputs.py, with no LDS
access outside the window assign_layout.h computes."""
import os
import subprocess

import numpy as np
import pytest

import assignment_inputs as ai

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_emu():
    """Builds tests/support/emu_assign.cpp (when stale) and returns run(text) -> its output lines without the OOB line."""
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "emu_assign")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    sup = os.path.join(ROOT, "tests", "support")
    deps = [os.path.join(sup, "emu_assign.cpp"), os.path.join(sup, "wave_emu_assign.h"), os.path.join(sup, "wave_emu.h"),
            os.path.join(csrc, "assign_wave.h"), os.path.join(csrc, "assign_layout.h"), os.path.join(csrc, "heur_layout.h"),
            os.path.join(csrc, "host", "assign_pack.h"), os.path.join(csrc, "host", "assign_series.h"),
            os.path.join(csrc, "host", "ll_pack.h"), os.path.join(ROOT, "include", "mrp_ll.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, deps[0]])

    def run(text):
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = r.stdout.split("\n")
        while lines and not lines[-1]:
            lines.pop()
        assert lines[-1] == "OOB 0 0", ("LDS access outside the window", lines[-1])
        return lines[:-1]
    return run


@pytest.fixture(scope="module")
def emu():
    return build_emu()


def solve_record(p):
    w = ["solve", p["nA"], p["nT"], p["min_matching"], int(p["mode"] is not None), int(p["forbidden"] is not None)]
    w += p["cost"].reshape(-1).tolist()
    w += p["mode"] or []
    w += p["forbidden"] or []
    return " ".join(str(x) for x in w)


def parse_result(line):
    f = line.split()
    assert f[0] == "R"
    return int(f[1]), int(f[2]), int(f[3]), [int(x) for x in f[4:]]


def solve_all(emu, problems):
    lines = emu("\n".join(solve_record(p) for p in problems) + "\n")
    assert len(lines) == len(problems)
    return [parse_result(l) for l in lines]


def assert_equals_brute(p, res, what):
    status, matched, cost, task_of = res
    K, best, _ = ai.brute(p)
    if K is None:
        assert (status, matched, cost) == (ai.INFEASIBLE, 0, 0), what
        assert all(t == -1 for t in task_of), what
    else:
        assert (status, matched, cost) == (ai.OK, K, best), (what, res, K, best)
        ai.check_matching(p, status, matched, cost, task_of)


def series_all(emu, problems):
    text = "".join("series %d %d %s\n" % (p["nA"], p["nT"], " ".join(str(x) for x in p["cost"].reshape(-1).tolist()))
                   for p in problems)
    lines = emu(text)
    out, k = [], 0
    for _ in problems:
        n = int(lines[k].split()[1])
        out.append([parse_result(l) for l in lines[k + 1:k + 1 + n]])
        k += 1 + n
    assert k == len(lines)
    return out


def assert_series_equals_brute(p, got, what):
    """Cost sequence = brute's sorted costs, set of matchings = brute's set (each once), then exhausted — three times."""
    K, _, at_k = ai.brute(p)
    assert [g[0] for g in got[-3:]] == [ai.INFEASIBLE] * 3 and all(g[1] == 0 for g in got[-3:]), what
    sols = got[:-3]
    assert all(s[0] == ai.OK and s[1] == K for s in sols), what
    assert [s[2] for s in sols] == [c for c, _ in at_k], (what, [s[2] for s in sols])
    assert sorted((s[2], tuple(s[3])) for s in sols) == at_k, what


def test_hungarian_yardstick_equals_brute():
    """The O(n^3) yardstick used beyond brute force agrees with the enumeration on 300 random problems up to 6 x 6."""
    for k, p in enumerate(ai.random_small(300, 11, constraints=False)):
        K, best, _ = ai.brute(p)
        assert ai.hungarian(p["cost"]) == (K, best), k


def test_four_by_four_facts():
    """What the issue states about the reference's 4 x 4, by enumeration."""
    K, best, at_k = ai.brute(ai.reference_cases()["4by4"])
    costs = [c for c, _ in at_k]
    assert (K, best, len(at_k)) == (4, 275, 24)
    assert at_k[0] == (275, (3, 2, 1, 0)) and at_k[-1] == (400, (2, 1, 0, 3))
    assert costs.count(275) == 1 and costs.count(400) == 1
    assert max(costs.count(c) for c in costs) == 2 and costs.count(355) == 2 and costs.count(375) == 2


def test_fixed_cases_equal_brute(emu):
    cases = dict(ai.small_cases())
    cases.update(ai.constraint_cases())
    names = sorted(cases)
    res = solve_all(emu, [cases[n] for n in names])
    for n, r in zip(names, res):
        assert_equals_brute(cases[n], r, n)
        assert (r[0] == ai.INFEASIBLE) == n.startswith("infeasible"), n
    by = dict(zip(names, res))
    assert by["2by1"][2:] == (1, [-1, 0]) and by["1by2"][2:] == (1, [1]) and by["empty"][:3] == (ai.OK, 0, 0)
    assert by["4by4"][2:] == (275, [3, 2, 1, 0])
    assert by["no_tasks"][:3] == (ai.OK, 0, 0) and by["no_agents"][:3] == (ai.OK, 0, 0)


def test_large_fixed_cases(emu):
    cases = ai.large_cases()
    names = sorted(cases)
    res = solve_all(emu, [cases[n][0] for n in names])
    for n, r in zip(names, res):
        p, K, cost = cases[n]
        assert r[:3] == (ai.OK, K, cost), (n, r[:3], K, cost)
        ai.check_matching(p, *r)
    assert dict(zip(names, res))["64by64_max_cost"][2] == 64 * 16777215


def test_random_small_equal_brute(emu):
    problems = ai.random_small(1000, 1)
    for k, (p, r) in enumerate(zip(problems, solve_all(emu, problems))):
        assert_equals_brute(p, r, k)


def test_random_large_equal_hungarian(emu):
    problems = ai.random_large(64, 2)
    for k, (p, r) in enumerate(zip(problems, solve_all(emu, problems))):
        assert r[:3] == (ai.OK,) + ai.hungarian(p["cost"]), k
        ai.check_matching(p, *r)


def test_task_of_equals_the_recorded_one(emu):
    """Determinism: the matchings themselves, not only their cost, are recorded in tests/golden/assign_task_of.json
    (written by tests/golden/make_assign_fixture.py from this emulator); tests/test_assign_gpu.py holds the device to the
    same file, so the emulator and the device give the same task_of."""
    want = ai.recorded_task_of()
    sets = ai.recorded_sets()
    assert sorted(want) == sorted(sets)
    for name in sorted(sets):
        got = solve_all(emu, sets[name])
        assert [[r[0], r[1], r[2], r[3]] for r in got] == want[name], name


def test_series_fixed_cases(emu):
    cases = ai.small_cases()
    names = sorted(cases)
    got = dict(zip(names, series_all(emu, [cases[n] for n in names])))
    for n in names:
        assert_series_equals_brute(cases[n], got[n], n)
    assert [(s[2], s[3]) for s in got["2by1"][:-3]] == [(1, [-1, 0]), (2, [0, -1])]
    four = got["4by4"][:-3]
    assert len(four) == 24 and (four[0][2], four[0][3]) == (275, [3, 2, 1, 0]) and (four[-1][2], four[-1][3]) == (400, [2, 1, 0, 3])
    assert len(got["empty"]) == 4 and got["empty"][0][:3] == (ai.OK, 0, 0)  # K = 0: the empty matching once


def test_series_random_equal_brute(emu):
    problems = ai.random_small(200, 3, max_dim=5, constraints=False)
    for k, (p, got) in enumerate(zip(problems, series_all(emu, problems))):
        assert_series_equals_brute(p, got, k)


def test_gather_form_equals_matrix_form(emu):
    """cost(a, t) read from heuristic tables laid out as the engine lays them (32 x 32: [y * 32 + x]; 48 x 48:
    [y * dimx + x]), with goals in a walled-off pocket (unreachable = no edge) and some pairs masked out."""
    cases = ai.gather_cases()
    records = []
    for g in cases:
        m = g["map"]
        w = ["gsolve", m["dimx"], m["dimy"], len(g["starts"]), len(g["goals"]), 0, 0, 0, 1]
        for t in g["tables"]:
            w += np.asarray(t, dtype=np.int64).reshape(-1).tolist()
        for s in g["starts"]:
            w += [s[0], s[1]]
        w += g["allowed"]
        records.append(" ".join(str(x) for x in w))
    got = [parse_result(l) for l in emu("\n".join(records) + "\n")]
    assert got == solve_all(emu, [g["problem"] for g in cases])
    for g, r in zip(cases, got):
        assert r[:3] == (ai.OK,) + ai.hungarian(g["problem"]["cost"])
        ai.check_matching(g["problem"], *r)
