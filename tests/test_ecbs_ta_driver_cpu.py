"""The batched ECBS-TA driver (csrc/hl/mrp_hl_ecbs_ta.cpp) built with g++ against the oracle-backed stand-in engine
(tests/support/mock_ll_ta_eps.cpp): equal to the sequential restatement on the whole corpus at every w — status, cost,
makespan, both counters, the assignments asked for, roots, tasks, schedule digest, end states — as one batch and one by one,
with roots as one call and as dependent jobs; the assignment limit, the high-level cap, the low-level budget, an empty batch."""
import functools
import os
import subprocess

import pytest

import ecbs_ta_tree_corpus as corpus

ROOT = corpus.ROOT
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
HL = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc", "hl")


@pytest.fixture(scope="module")
def driver(oracle_mod):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libmrp_hl_cpu_ecbs_ta.so")
    srcs = [os.path.join(HL, "mrp_hl.cpp"), os.path.join(HL, "mrp_hl_ta.cpp"), os.path.join(HL, "mrp_hl_ecbs_ta.cpp"),
            os.path.join(SUPPORT, "mock_ll_ta_eps.cpp"), os.path.join(SUPPORT, "mock_ll_ta_assign.cpp"),
            os.path.join(SUPPORT, "ecbs_ta_check.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "oracle"), "-I", SUPPORT, "-o", out] + srcs +
                          ["-Wl,--wrap=mrp_ll_search_batch", "-L", os.path.join(ROOT, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return out


@pytest.mark.parametrize("use_root_kernel", [0, 1])
@pytest.mark.parametrize("w", corpus.WS)
def test_driver_equals_the_restatement(driver, ref_tests, w, use_root_kernel):
    from libmultirobotplanning_amd import hl
    named = corpus.ref_inputs(ref_tests)
    insts = corpus.corpus() + list(named.values())
    got, stats = hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=bool(use_root_kernel), _lib_path=driver)
    for g, i in zip(got, insts):
        corpus.same(g, corpus.reference(i, w))
    if w == 1.0:
        assert [g["cost"] for g in got[-3:]] == [6, 6, 5]
    assert stats["solved"] == len(insts) and stats["ll_searches"] == sum(g["n_ll_searches"] for g in got)
    # a root is one search per agent, and only whole roots are pushed here (no root search fails without a budget)
    for g, i in zip(got, insts):
        assert g["n_root_searches"] == g["n_roots"] * len(i["starts"])


@pytest.mark.parametrize("use_root_kernel", [0, 1])
def test_one_by_one_equals_the_batch(driver, use_root_kernel):
    from libmultirobotplanning_amd import hl
    for inst, w in corpus.pairs():
        got, stats = hl.solve_ecbs_ta_batch([inst], w, use_root_kernel=bool(use_root_kernel), _lib_path=driver)
        corpus.same(got[0], corpus.reference(inst, w))
        assert stats["rounds"] >= (1 if use_root_kernel else len(inst["starts"]))  # roots as jobs: one agent per round


def test_a_round_is_at_most_one_call_of_each_kind(driver, tmp_path, monkeypatch):
    from libmultirobotplanning_amd import hl
    log = tmp_path / "calls.txt"
    monkeypatch.setenv("MRP_MOCK_TA_CALLS", str(log))
    _, stats = hl.solve_ecbs_ta_batch(corpus.corpus(), 1.3, use_root_kernel=True, _lib_path=driver)
    calls = log.read_text().split()
    assert calls.count("compute_heuristics") == 1 and calls.count("assign_series_create") == 1
    assert calls.count("ta_root_batch") == 0
    for name in ("assign_series_next", "ta_eps_root_batch", "search_batch"):
        assert 1 <= calls.count(name) <= stats["rounds"], (name, calls.count(name), stats["rounds"])
    rounds_with_call = stats["rounds"]
    log.write_text("")
    _, stats = hl.solve_ecbs_ta_batch(corpus.corpus(), 1.3, use_root_kernel=False, _lib_path=driver)
    calls = log.read_text().split()
    assert calls.count("ta_eps_root_batch") == 0 and 1 <= calls.count("search_batch") <= stats["rounds"]
    assert stats["rounds"] > rounds_with_call  # a root as jobs is one dependent round per agent


@pytest.mark.parametrize("use_root_kernel", [0, 1])
def test_limits(driver, use_root_kernel):
    from libmultirobotplanning_amd import hl
    insts = corpus.corpus()
    solve = functools.partial(hl.solve_ecbs_ta_batch, use_root_kernel=bool(use_root_kernel), _lib_path=driver)
    for w in (1.0, 1.3):
        for max_ta in (0, 1):  # m_maxTaskAssignments with the reference's `>` (ecbs_ta.cpp:514)
            got, _ = solve(insts, w, max_task_assignments=max_ta)
            for g, i in zip(got, insts):
                corpus.same(g, corpus.reference(i, w, max_task_assignments=max_ta))
                assert g["num_task_assignments"] <= max_ta + 1
        refs = [corpus.reference(i, w) for i in insts]
        deep = max(range(len(insts)), key=lambda q: refs[q]["hl_expanded"])
        cap = refs[deep]["hl_expanded"] - 1
        assert cap >= 1
        got, _ = solve(insts, w, max_hl_expansions=cap)
        assert got[deep]["status"] == hl.CAP and got[deep]["hl_expanded"] == cap
        for g, i, r in zip(got, insts, refs):
            corpus.same(g, r if r["hl_expanded"] <= cap else corpus.reference(i, w, max_hl=cap))
    # the low-level budget: an instance that needs more ends MRP_HL_CAP, the others are untouched
    refs = [corpus.reference(i, 1.3) for i in insts]
    budget = sorted(r["ll_expanded"] for r in refs)[len(refs) // 2]
    got, _ = solve(insts, 1.3, max_ll_expansions=budget)
    assert any(g["status"] == hl.CAP for g in got)
    for g, r in zip(got, refs):
        if r["ll_expanded"] <= budget:
            corpus.same(g, r)
        else:
            assert g["status"] == hl.CAP and g["paths"] is None


def test_empty_batch_bad_weight_and_nobody_with_a_task(driver):
    from libmultirobotplanning_amd import hl
    assert hl.solve_ecbs_ta_batch([], 1.3, _lib_path=driver)[0] == []
    inst = corpus.instance(0)
    with pytest.raises(RuntimeError):
        hl.solve_ecbs_ta_batch([inst], 0.5, _lib_path=driver)
    # nobody can be assigned anything: the first root is planned without tasks, and nobody moves
    nothing = dict(dimx=4, dimy=4, obstacles=[], starts=[[0, 0], [1, 1]], potential_goals=[[], []])
    for k in (False, True):
        got, _ = hl.solve_ecbs_ta_batch([nothing], 1.3, use_root_kernel=k, _lib_path=driver)
        corpus.same(got[0], corpus.reference(nothing, 1.3))
        assert got[0]["status"] == hl.SOLVED and got[0]["cost"] == 0 and got[0]["num_task_assignments"] == 0
        assert got[0]["tasks"] == [None, None] and got[0]["n_ll_searches"] == 2
