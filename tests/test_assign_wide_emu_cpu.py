"""The wide assignment wave program (libmultirobotplanning_amd/csrc/assign_wave_wide.h — the source the gfx950 kernel
compiles, up to 256 agents x 256 tasks) on the CPU: tests/support/emu_assign_wide.cpp builds it against the 64-lane
lockstep interpretation of its wave vocabulary, behind the engine's wide packer and the generalised next-best series, as a
program of its own under -fsanitize=address,undefined.  Every staged area is a heap block of exactly its size and there
must be no LDS access outside the window.  Both row sources run: the LDS budget is an input (65536: the default; 0: every
problem reads its rows from memory)."""
import os
import subprocess

import numpy as np
import pytest

import assignment_inputs as ai
import assignment_wide_inputs as wi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = (65536, 0)  # LDS rows wherever they fit (the default) / memory rows for every problem


def build_emu():
    """Builds tests/support/emu_assign_wide.cpp (when stale) and returns run(text) -> its output lines without the OOB line."""
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "emu_assign_wide")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    sup = os.path.join(ROOT, "tests", "support")
    deps = [os.path.join(sup, "emu_assign_wide.cpp"), os.path.join(sup, "wave_emu_assign.h"), os.path.join(sup, "wave_emu.h"),
            os.path.join(csrc, "assign_wave_wide.h"), os.path.join(csrc, "assign_wave.h"), os.path.join(csrc, "assign_layout.h"),
            os.path.join(csrc, "heur_layout.h"), os.path.join(csrc, "host", "assign_pack.h"),
            os.path.join(csrc, "host", "assign_series.h"), os.path.join(csrc, "host", "ll_pack.h"),
            os.path.join(ROOT, "include", "mrp_ll.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, deps[0]])

    def run(text):
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=900)
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


def mask_words(p):
    return max(1, (p["nT"] + 63) // 64)


def solve_record(p):
    mw = mask_words(p) if p["forbidden"] is not None else 0
    w = ["solve", p["nA"], p["nT"], p["min_matching"], int(p["mode"] is not None), mw]
    w += p["cost"].reshape(-1).tolist()
    w += p["mode"] or []
    for f in p["forbidden"] or []:
        w += [(f >> (64 * k)) & (2 ** 64 - 1) for k in range(mw)]
    return " ".join(map(str, w))


def narrow_record(p):
    w = ["narrow", p["nA"], p["nT"], p["min_matching"], int(p["mode"] is not None), int(p["forbidden"] is not None)]
    w += p["cost"].reshape(-1).tolist()
    w += p["mode"] or []
    w += p["forbidden"] or []
    return " ".join(map(str, w))


def sparse_record(p):
    a, t = np.nonzero(p["cost"] != ai.NO_EDGE)
    w = ["sparse", p["nA"], p["nT"], p["min_matching"], len(a)]
    for x, y in zip(a.tolist(), t.tolist()):
        w += [x, y, int(p["cost"][x, y])]
    modes = [(i, m) for i, m in enumerate(p["mode"] or []) if m != ai.FREE]
    w += [len(modes)] + [v for pair in modes for v in pair]
    forb = [(i, b) for i, f in enumerate(p["forbidden"] or []) for b in range(p["nT"]) if (f >> b) & 1]
    w += [len(forb)] + [v for pair in forb for v in pair]
    return " ".join(map(str, w))


def parse_result(line):
    f = line.split()
    assert f[0] == "R"
    return int(f[1]), int(f[2]), int(f[3]), [int(x) for x in f[4:]]


def solve_all(emu, problems, budget, record=solve_record):
    lines = emu("budget %d\n" % budget + "\n".join(record(p) for p in problems) + "\n")
    assert len(lines) == len(problems)
    return [parse_result(l) for l in lines]


@pytest.fixture(scope="module")
def recorded_results(emu):
    """The groups the golden file records (shapes, constraints beyond bit 63), solved under both row sources."""
    probs = dict(wi.shape_problems())
    probs.update({n: p for n, (p, _) in wi.constraint_problems().items()})
    names = wi.recorded_names()
    return {b: dict(zip(names, solve_all(emu, [probs[n] for n in names], b))) for b in BUDGETS}


@pytest.mark.parametrize("budget", BUDGETS)
def test_narrow_sets_equal_the_recorded_task_of(emu, budget):
    """With nA, nT <= 64 the wide program is the narrow one, task_of entry for entry: the narrow golden file."""
    want, sets = ai.recorded_task_of(), ai.recorded_sets()
    for name in sorted(sets):
        got = solve_all(emu, sets[name], budget)
        assert [[r[0], r[1], r[2], r[3]] for r in got] == want[name], name


@pytest.mark.parametrize("budget", BUDGETS)
def test_random_small_equals_the_narrow_emulator(emu, budget):
    problems = ai.random_small(1000, 1)
    narrow = [parse_result(l) for l in emu("\n".join(narrow_record(p) for p in problems) + "\n")]
    assert solve_all(emu, problems, budget) == narrow


@pytest.mark.parametrize("budget", BUDGETS)
def test_embedded_small_equal_brute(emu, budget):
    """Small problems on agent and task indices up to 255: (status, K, cost) is brute force's on the small problem."""
    pairs = wi.embedded_small()
    got = solve_all(emu, [big for _, big in pairs], budget, sparse_record)
    for k, ((small, big), r) in enumerate(zip(pairs, got)):
        K, best, _ = ai.brute(small)
        if K is None:
            assert r[:3] == (ai.INFEASIBLE, 0, 0) and all(t == -1 for t in r[3]), k
        else:
            assert r[:3] == (ai.OK, K, best), (k, r[:3], K, best)
            ai.check_matching(big, *r)


def test_embedded_series_equal_brute(emu):
    """The whole next-best series of 30 embedded problems: brute force's multiset of (cost, matching), costs
    non-decreasing, then NO_SOLUTION three times."""
    cases = wi.embedded_series()
    assert len(cases) == 30
    text = "".join("series %d %d %s\n" % (big["nA"], big["nT"], " ".join(map(str, big["cost"].reshape(-1).tolist())))
                   for _, big, _, _ in cases)
    lines = emu(text)
    k = 0
    for n, (small, big, ag, tk) in enumerate(cases):
        cnt = int(lines[k].split()[1])
        got = [parse_result(l) for l in lines[k + 1:k + 1 + cnt]]
        k += 1 + cnt
        K, _, at_k = ai.brute(small)
        assert [g[0] for g in got[-3:]] == [ai.INFEASIBLE] * 3 and all(g[1] == 0 for g in got[-3:]), n
        sols = got[:-3]
        assert all(s[0] == ai.OK and s[1] == K for s in sols), n
        assert [s[2] for s in sols] == [c for c, _ in at_k], n
        back = {t: i for i, t in enumerate(tk)}
        small_matchings = []
        for s in sols:
            assert all(t == -1 for a, t in enumerate(s[3]) if a not in ag), n
            small_matchings.append((s[2], tuple(back.get(s[3][a], -1) for a in ag)))
        assert sorted(small_matchings) == at_k, n
    assert k == len(lines)


def test_shapes_equal_hungarian_under_both_row_sources(recorded_results):
    probs = wi.shape_problems()
    for name, p in probs.items():
        r = recorded_results[BUDGETS[0]][name]
        assert r[:3] == wi.expected(name, (p["cost"], 0, 0)), (name, r[:3])
        ai.check_matching(p, *r)
        assert recorded_results[BUDGETS[1]][name] == r, name


@pytest.mark.parametrize("budget", BUDGETS)
def test_numbers_at_256_by_256_max_cost(emu, budget):
    """256 pairs of 2^24 - 1 each: 2^32 - 256 = 4 294 967 040, below the no-task price 2^32."""
    r = solve_all(emu, [wi.max_cost_problem()], budget)[0]
    assert 256 * ai.MAX_COST == 4294967040 == 2 ** 32 - 256
    assert r[:3] == (ai.OK, 256, 4294967040)


def test_constraints_beyond_bit_63(recorded_results):
    for name, (p, expectation) in wi.constraint_problems().items():
        r = recorded_results[BUDGETS[0]][name]
        assert (expectation is None) == name.startswith("infeasible")
        assert r[:3] == wi.expected(name, expectation), (name, r[:3])
        if expectation is None:
            assert all(t == -1 for t in r[3]) and len(r[3]) == p["nA"]
        else:
            ai.check_matching(p, *r)
        assert recorded_results[BUDGETS[1]][name] == r, name
    by = recorded_results[BUDGETS[0]]
    assert by["forced_255"][3][3] == 255
    assert by["forbidden_64_127_128_255"][3][0] not in (64, 127, 128, 255)


def test_task_of_equals_the_recorded_one(recorded_results):
    """tests/golden/assign_wide_task_of.json (written by tests/golden/make_assign_wide_fixture.py from this emulator)
    holds these matchings; tests/test_assign_wide_gpu.py holds the device to the same file."""
    want = wi.recorded_task_of()
    assert sorted(want) == wi.recorded_names()
    for name in wi.recorded_names():
        assert list(recorded_results[BUDGETS[0]][name]) == want[name], name


def test_gather_form_equals_matrix_form(emu):
    """cost(a, t) read from heuristic tables (a 12 x 11 map, 70 tasks and 66 agents: two column slots per lane), some pairs
    masked out through a 2-word `allowed`, some table entries unreachable — against the same problem as a matrix, under
    both row sources (memory rows: the wave writes the matrix into its scratch region first)."""
    rng = np.random.RandomState(31)
    dimx, dimy, nA, nT = 12, 11, 66, 70
    tables = rng.randint(0, 40, size=(nT, dimy, dimx))
    tables[rng.rand(nT, dimy, dimx) < 0.1] = -1
    starts = [(int(rng.randint(0, dimx)), int(rng.randint(0, dimy))) for _ in range(nA)]
    allowed = [sum(1 << t for t in range(nT) if rng.rand() < 0.8) for _ in range(nA)]
    cost = np.array([[ai.NO_EDGE if not (allowed[a] >> t) & 1 or tables[t][s[1], s[0]] < 0 else int(tables[t][s[1], s[0]])
                      for t in range(nT)] for a, s in enumerate(starts)], dtype=np.int64)
    w = ["gsolve", dimx, dimy, nA, nT, 2] + tables.reshape(-1).tolist() + [v for s in starts for v in s]
    for m in allowed:
        w += [m & (2 ** 64 - 1), m >> 64]
    p = ai.problem(cost)
    want = solve_all(emu, [p], BUDGETS[0])[0]
    assert want[:3] == (ai.OK,) + ai.hungarian(cost)
    ai.check_matching(p, *want)
    for b in BUDGETS:
        got = [parse_result(l) for l in emu("budget %d\n%s\n" % (b, " ".join(map(str, w))))]
        assert got == [want], b
