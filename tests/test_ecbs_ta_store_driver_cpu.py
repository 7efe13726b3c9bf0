"""The batched ECBS-TA driver under MRP_HL_TA_DEVICE_PATHS=1 (csrc/hl/mrp_hl_ecbs_ta.cpp) built with g++ against a stand-in
engine that keeps a path per store slot (tests/support/mock_ll_ta_eps_store.cpp): with the knob on every instance of the
corpus equals the sequential restatement and the knob-off run, at every w and with both root forms; jobs go out by slot;
a store so small that the free list runs dry gives the same answers with both forms of job; the limits hold.  The stand-in
refuses a job that names a slot nobody wrote, a slot rewritten since, or a slot written in the same batch, so a mistake in
a slot's lifetime ends an instance MRP_HL_LL_ERROR instead of passing."""
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
    out = os.path.join(BUILD, "libmrp_hl_cpu_ecbs_ta_store.so")
    srcs = [os.path.join(HL, "mrp_hl.cpp"), os.path.join(HL, "mrp_hl_ta.cpp"), os.path.join(HL, "mrp_hl_ecbs_ta.cpp"),
            os.path.join(SUPPORT, "mock_ll_ta_eps_store.cpp"), os.path.join(SUPPORT, "mock_ll_ta_assign.cpp"),
            os.path.join(SUPPORT, "ecbs_ta_check.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "oracle"), "-I", SUPPORT, "-o", out] + srcs +
                          ["-Wl,--wrap=mrp_ll_search_batch", "-L", os.path.join(ROOT, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return out


def _stats(s):
    return {k: v for k, v in s.items() if "seconds" not in k and not k.endswith("_ms")}


@pytest.fixture(scope="module")
def knob_off(driver, ref_tests):
    """(instances, {(w, use_root_kernel): (solutions, stats)}) with the knob unset."""
    from libmultirobotplanning_amd import hl
    assert "MRP_HL_TA_DEVICE_PATHS" not in os.environ
    insts = corpus.corpus() + list(corpus.ref_inputs(ref_tests).values())
    return insts, {(w, k): hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=bool(k), _lib_path=driver) for w in corpus.WS for k in (0, 1)}


@pytest.mark.parametrize("use_root_kernel", [0, 1])
@pytest.mark.parametrize("w", corpus.WS)
def test_knob_on_equals_the_restatement_and_the_knob_off_run(driver, knob_off, tmp_path, monkeypatch, w, use_root_kernel):
    from libmultirobotplanning_amd import hl
    insts, off = knob_off
    log = tmp_path / "calls.txt"
    monkeypatch.setenv("MRP_MOCK_TA_CALLS", str(log))
    monkeypatch.setenv("MRP_HL_TA_DEVICE_PATHS", "1")
    got, stats = hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=bool(use_root_kernel), _lib_path=driver)
    for g, i in zip(got, insts):
        corpus.same(g, corpus.reference(i, w))
    assert got == off[(w, use_root_kernel)][0]
    assert _stats(stats) == _stats(off[(w, use_root_kernel)][1])
    calls = log.read_text().split()
    assert calls.count("path_store_reserve") == 1
    # every context goes by slot: with the default store no search of this corpus finds the free list empty
    assert calls.count("job_by_id") >= 50 and calls.count("job_shipped") == 0
    for name in ("assign_series_next", "search_batch"):
        assert 1 <= calls.count(name) <= stats["rounds"]
    roots = calls.count("ta_eps_root_batch")
    assert (1 <= roots <= stats["rounds"]) if use_root_kernel else roots == 0


@pytest.mark.parametrize("use_root_kernel", [0, 1])
def test_a_store_that_runs_dry_mixes_both_forms_of_job(driver, knob_off, tmp_path, monkeypatch, use_root_kernel):
    from libmultirobotplanning_amd import hl
    insts, off = knob_off
    log = tmp_path / "calls.txt"
    monkeypatch.setenv("MRP_MOCK_TA_CALLS", str(log))
    monkeypatch.setenv("MRP_HL_TA_DEVICE_PATHS", "1")
    monkeypatch.setenv("MRP_HL_TA_PATH_SLOTS", "60")  # fewer than the corpus's roots need: the trees behind the first few ship
    got, stats = hl.solve_ecbs_ta_batch(insts, 1.3, use_root_kernel=bool(use_root_kernel), _lib_path=driver)
    assert got == off[(1.3, use_root_kernel)][0] and _stats(stats) == _stats(off[(1.3, use_root_kernel)][1])
    calls = log.read_text().split()
    assert calls.count("job_by_id") >= 1 and calls.count("job_shipped") >= 1


@pytest.mark.parametrize("use_root_kernel", [0, 1])
def test_limits_with_the_knob_on(driver, monkeypatch, use_root_kernel):
    """As test_ecbs_ta_driver_cpu.py test_limits, at w = 1.3: the high-level cap and the low-level budget (searches that end
    at the budget leave no path: their slots go back)."""
    from libmultirobotplanning_amd import hl
    monkeypatch.setenv("MRP_HL_TA_DEVICE_PATHS", "1")
    insts, w = corpus.corpus(), 1.3

    def solve(**kw):
        return hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=bool(use_root_kernel), _lib_path=driver, **kw)
    refs = [corpus.reference(i, w) for i in insts]
    deep = max(range(len(insts)), key=lambda q: refs[q]["hl_expanded"])
    cap = refs[deep]["hl_expanded"] - 1
    assert cap >= 1
    got, _ = solve(max_hl_expansions=cap)
    assert got[deep]["status"] == hl.CAP and got[deep]["hl_expanded"] == cap
    for g, i, r in zip(got, insts, refs):
        corpus.same(g, r if r["hl_expanded"] <= cap else corpus.reference(i, w, max_hl=cap))
    budget = sorted(r["ll_expanded"] for r in refs)[len(refs) // 2]
    got, _ = solve(max_ll_expansions=budget)
    assert any(g["status"] == hl.CAP for g in got)
    for g, r in zip(got, refs):
        if r["ll_expanded"] <= budget:
            corpus.same(g, r)
        else:
            assert g["status"] == hl.CAP and g["paths"] is None
