"""Host-side logic (csrc/hl/: CT state machines, exact HL heaps, conflict scans, batching) on a machine without a GPU.

The drivers are compiled with g++ against tests/support/mock_ll.cpp — a TEST-ONLY stand-in for libmrp_ll.so that answers
every low-level job with the oracle's search — and must reproduce the oracle's whole-instance results.  This isolates
the host logic from the kernel; the product library itself has no CPU path (see test_library_exports.py).
"""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")


ROOT_CHAIN_NAMES = ["map_32by32_obst204_agents10_ex%d" % k for k in range(0, 40, 3)] + [
    "map_32by32_obst204_agents20_ex1", "map_32by32_obst204_agents30_ex2"]


def _digest(paths):
    h = hashlib.sha256()
    for p in paths:
        h.update(("|" + ",".join("%d:%d" % (x, y) for x, y in p)).encode())
    return h.hexdigest()[:16]


@pytest.fixture(scope="module")
def cpu_solver(oracle_mod):
    from libmultirobotplanning_amd import hl
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libmrp_hl_cpu.so")
    srcs = [os.path.join(ROOT, "libmultirobotplanning_amd", "csrc", "hl", "mrp_hl.cpp"),
            os.path.join(ROOT, "tests", "support", "mock_ll.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-o", out] + srcs + ["-L", os.path.join(ROOT, "oracle"), "-loracle",
                                                "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    s = hl.BatchSolver(device=0, n_threads=3, _lib_path=out)
    yield s
    s.close()


def test_known_answers(cpu_solver, ref_tests):
    from libmultirobotplanning_amd import hl
    names = ["mapf_simple1", "mapf_circle", "mapf_atGoal"]
    insts = [ref_tests["mapf"][n] for n in names]
    res, _ = cpu_solver.solve(insts, algo=hl.CBS)
    assert [r["cost"] for r in res] == [ref_tests["cbs_cost"][n] for n in names]
    res, _ = cpu_solver.solve(insts, algo=hl.ECBS, w=1.0)
    assert [r["cost"] for r in res] == [ref_tests["ecbs_w1_cost"][n] for n in names]


def test_ecbs_batch_matches_oracle(cpu_solver, bench_instances, oracle_expected):
    from libmultirobotplanning_amd import hl
    names = [n for n in sorted(bench_instances) if "32by32" in n and ("agents10_" in n or "agents20_" in n
                                                                     or "agents30_" in n)][:60]
    names += ["map_32by32_obst204_agents50_ex0", "map_32by32_obst204_agents100_ex0"]
    res, stats = cpu_solver.solve([bench_instances[n] for n in names], algo=hl.ECBS, w=1.3)
    for n, r in zip(names, res):
        e = oracle_expected[n]["ecbs_w1.3"]
        assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"]) == (
            hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"]), n
        assert _digest(r["paths"]) == e["digest"], n
    assert stats["ll_expansions"] == sum(r["ll_expanded"] for r in res)


def test_stream_of_batches_equals_separate_solves(cpu_solver, bench_instances, oracle_expected):
    """mrp_hl_solver_solve_stream: three prepared batches (one of them empty-handed: a single instance) drawn from one pool
    without a barrier between them give, batch by batch, exactly what their own solve_prepared calls give — the oracle's
    results, schedules included — and the stream's statistics are the sums."""
    from libmultirobotplanning_amd import hl
    names = [n for n in sorted(bench_instances) if "32by32" in n and ("agents10_" in n or "agents20_" in n)][:50]
    groups = [names[:30], names[30:31], names[31:]]
    preps = [cpu_solver.prepare([bench_instances[n] for n in g], want_paths=True, path_cap=256) for g in groups]
    try:
        st = cpu_solver.solve_stream(preps, algo=hl.ECBS, w=1.3)
        total = 0
        for g, prep in zip(groups, preps):
            for n, r in zip(g, cpu_solver.results_of(prep)):
                e = oracle_expected[n]["ecbs_w1.3"]
                assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"]) == (
                    hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"]), n
                assert _digest(r["paths"]) == e["digest"], n
                total += r["ll_expanded"]
        assert st["ll_expansions"] == total and st["solved"] == len(names) and st["batches"] == 3
        # CBS (its own session kernels, independent root searches, no path store), mixed map sizes, an EMPTY batch in the middle
        cn = [n for n in sorted(bench_instances) if "8by8" in n and oracle_expected[n]["cbs"]["rc"] == 1]
        cgroups = [cn[:5], [], cn[5:]]
        cpreps = [cpu_solver.prepare([bench_instances[n] for n in g], want_paths=True, path_cap=256) for g in cgroups]
        try:
            cst = cpu_solver.solve_stream(cpreps, algo=hl.CBS)
            for g, prep in zip(cgroups, cpreps):
                for n, r in zip(g, cpu_solver.results_of(prep)):
                    e = oracle_expected[n]["cbs"]
                    assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"]) == (
                        hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"]), n
                    assert _digest(r["paths"]) == e["digest"], n
            assert cst["solved"] == len(cn)
        finally:
            for prep in cpreps:
                cpu_solver.release(prep)
        # the rounds schedule keeps a barrier between batches by construction: several batches are refused, not mis-served
        with pytest.raises(RuntimeError):
            opt_mode = cpu_solver._lib.mrp_hl_solver_solve_stream  # noqa: F841  (the binding exists)
            os.environ["MRP_HL_STATIC_SPLIT"] = "1"
            try:
                cpu_solver.solve_stream(preps, algo=hl.ECBS, w=1.3)
            finally:
                del os.environ["MRP_HL_STATIC_SPLIT"]
    finally:
        for prep in preps:
            cpu_solver.release(prep)


def test_co_workers_share_an_engine(cpu_solver, bench_instances, oracle_expected):
    """Five worker threads on two engines (mrp_ll_submit_tagged / mrp_ll_poll_any_tagged: two or three... two co-workers per
    engine, the fifth thread stays out): same results, every instance solved exactly once."""
    from libmultirobotplanning_amd import hl
    names = [n for n in sorted(bench_instances) if "32by32" in n and ("agents10_" in n or "agents20_" in n)][:80]
    os.environ["MRP_HL_MAX_ENGINES"] = "2"
    try:
        s = hl.BatchSolver(device=0, n_threads=5, _lib_path=os.path.join(BUILD, "libmrp_hl_cpu.so"))
    finally:
        del os.environ["MRP_HL_MAX_ENGINES"]
    try:
        for rep in range(2):
            res, stats = s.solve([bench_instances[n] for n in names], algo=hl.ECBS, w=1.3)
            for n, r in zip(names, res):
                e = oracle_expected[n]["ecbs_w1.3"]
                assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"]) == (
                    hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"]), n
                assert _digest(r["paths"]) == e["digest"], n
            assert stats["ll_expansions"] == sum(r["ll_expanded"] for r in res)
    finally:
        s.close()


def test_cbs_batch_matches_oracle(cpu_solver, bench_instances, oracle_expected):
    from libmultirobotplanning_amd import hl
    names = [n for n in sorted(bench_instances) if "8by8" in n and oracle_expected[n]["cbs"]["rc"] == 1]
    res, _ = cpu_solver.solve([bench_instances[n] for n in names], algo=hl.CBS)
    for n, r in zip(names, res):
        e = oracle_expected[n]["cbs"]
        assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"]) == (
            hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"]), n
        assert _digest(r["paths"]) == e["digest"], n


def test_caps_and_empty(cpu_solver, bench_instances, oracle_expected):
    from libmultirobotplanning_amd import hl
    hard = [n for n in sorted(bench_instances) if "8by8" in n and oracle_expected[n]["cbs"]["rc"] == -1][:2]
    res, _ = cpu_solver.solve([bench_instances[n] for n in hard], algo=hl.CBS, max_ll_expansions=5000)
    assert all(r["status"] == hl.CAP for r in res)
    res, _ = cpu_solver.solve([bench_instances[n] for n in hard], algo=hl.CBS, max_hl_expansions=10)
    assert all(r["status"] == hl.CAP and r["hl_expanded"] == 11 for r in res)
    res, stats = cpu_solver.solve([], algo=hl.ECBS)
    assert res == [] and stats["rounds"] == 0


def test_generator_is_deterministic_and_well_formed():
    from libmultirobotplanning_amd import hl
    a = hl.generate_instance(10007, 32, 32, 204, 10)
    b = hl.generate_instance(10007, 32, 32, 204, 10)
    assert a == b
    obst = {tuple(o) for o in a["obstacles"]}
    assert len(obst) == 204
    assert len({tuple(s) for s in a["starts"]}) == 10 and len({tuple(g) for g in a["goals"]}) == 10
    assert not (obst & {tuple(s) for s in a["starts"]}) and not (obst & {tuple(g) for g in a["goals"]})
    # every goal reachable from its start (4-connected)
    free = {(x, y) for x in range(32) for y in range(32)} - obst
    for s, g in zip(a["starts"], a["goals"]):
        seen, todo = {tuple(s)}, [tuple(s)]
        while todo:
            x, y = todo.pop()
            for c in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                if c in free and c not in seen:
                    seen.add(c)
                    todo.append(c)
        assert tuple(g) in seen


def test_linear_conflict_scans_match_quadratic_restatement():
    """grid_mapf.hpp's O(T*N) getFirstConflict / focalHeuristic scans vs the quadratic restatements of
    ecbs.cpp:401-452 / :315-350 on 100k random collision-rich path sets (tests/support/conflict_scan_check.cpp)."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "conflict_scan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe,
                           os.path.join(ROOT, "tests", "support", "conflict_scan_check.cpp")])
    out = subprocess.check_output([exe, "100000"], timeout=300).decode()
    assert out.strip() == "ok 100000", out


def test_speculative_expansion_changes_nothing_but_the_schedule(cpu_solver, bench_instances, oracle_expected, monkeypatch):
    """ct_solver.hpp "speculative expansion": for every look-ahead width, and with the groups of an instance coming back
    in scrambled order, CBS and ECBS give the sequential loop's (cost, makespan, HL, LL, paths); widths > 1 do issue
    searches ahead of their node's pop."""
    from libmultirobotplanning_amd import hl
    cbs_names = [n for n in sorted(bench_instances) if "8by8" in n and oracle_expected[n]["cbs"]["rc"] == 1
                 and oracle_expected[n]["cbs"]["ll"] < 60000]
    ecbs_names = [n for n in sorted(bench_instances) if "32by32" in n and ("agents30_" in n or "agents50_ex1" in n)]
    ecbs_names += ["map_32by32_obst204_agents100_ex0", "map_8by8_obst12_agents16_ex0", "map_8by8_obst12_agents16_ex1"]
    for spec, shuffle in ((1, None), (2, "3"), (4, None), (4, "1"), (16, "2")):
        monkeypatch.setenv("MRP_HL_SPEC", str(spec))
        if shuffle is None:
            monkeypatch.delenv("MRP_MOCK_SHUFFLE", raising=False)
        else:
            monkeypatch.setenv("MRP_MOCK_SHUFFLE", shuffle)
        res, st = cpu_solver.solve([bench_instances[n] for n in cbs_names], algo=hl.CBS)
        for n, r in zip(cbs_names, res):
            e = oracle_expected[n]["cbs"]
            assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"], _digest(r["paths"])) == (
                hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"], e["digest"]), (n, spec, shuffle)
        assert st["ll_expansions"] == sum(r["ll_expanded"] for r in res)
        assert (st["speculative_searches"] > 0) == (spec > 1)
        assert st["wasted_ll_expansions"] >= 0 and (spec > 1 or st["wasted_ll_expansions"] == 0)
        res, st = cpu_solver.solve([bench_instances[n] for n in ecbs_names], algo=hl.ECBS, w=1.3)
        for n, r in zip(ecbs_names, res):
            e = oracle_expected[n]["ecbs_w1.3"]
            assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"], _digest(r["paths"])) == (
                hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"], e["digest"]), (n, spec, shuffle)
        # caps behave the same whatever the width
        deep = [n for n in cbs_names if oracle_expected[n]["cbs"]["hl"] > 20][:3]
        assert len(deep) == 3
        res, _ = cpu_solver.solve([bench_instances[n] for n in deep], algo=hl.CBS, max_hl_expansions=7)
        assert all(r["status"] == hl.CAP and r["hl_expanded"] == 8 for r in res)


def test_root_chains_on_the_mock(cpu_solver, bench_instances, oracle_expected, monkeypatch):
    """The drivers' root chains (MRP_LL_JOB_ROOT_CHAIN) on the CPU: the mock keeps a host-side path store and runs a chain
    through the oracle; with MRP_MOCK_CHAIN_BREAK a search of more than that many expansions ends its chain in front of
    it, as a search that outgrows the LDS tier does on the device — the driver must run it as its own job and chain on."""
    from libmultirobotplanning_amd import hl
    names = ROOT_CHAIN_NAMES
    lib = os.path.join(BUILD, "libmrp_hl_cpu.so")
    monkeypatch.setenv("MRP_MOCK_PATH_STORE", "1")
    # "chunks": the root step in jobs of three searches (mrp_ll_job.chain_count; the drivers do this from 64 agents on)
    for brk in (None, "150", "0", "chunks"):
        monkeypatch.delenv("MRP_HL_CHAIN_CHUNK", raising=False)
        monkeypatch.delenv("MRP_HL_CHAIN_CHUNK_FROM", raising=False)
        if brk is None or brk == "chunks":
            monkeypatch.delenv("MRP_MOCK_CHAIN_BREAK", raising=False)
        else:
            monkeypatch.setenv("MRP_MOCK_CHAIN_BREAK", brk)
        if brk == "chunks":
            monkeypatch.setenv("MRP_HL_CHAIN_CHUNK", "3")
            monkeypatch.setenv("MRP_HL_CHAIN_CHUNK_FROM", "2")
        s = hl.BatchSolver(device=0, n_threads=2, _lib_path=lib)
        try:
            res, st = s.solve([bench_instances[n] for n in names], algo=hl.ECBS, w=1.3)
        finally:
            s.close()
        searches = 0
        for n, r in zip(names, res):
            e = oracle_expected[n]["ecbs_w1.3"]
            assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"]) == (
                hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"]), (n, brk)
            assert _digest(r["paths"]) == e["digest"], (n, brk)
            searches += r["ll_searches"]
        # chains: far fewer tickets than searches; "0": every chain breaks at its first search, one ticket more per search
        if brk is None:
            assert st["rounds"] * 3 < searches
            # conflict-free roots (the chain's own scan says so) are written without a conflict tree
            assert st["root_solved"] == sum(1 for r in res if r["hl_expanded"] == 1) > 0
        if brk == "0":
            assert st["rounds"] > searches
        if brk == "chunks":  # ten agents = four jobs (3 + 3 + 3 + 1) instead of one: more tickets than whole chains, far fewer than searches
            assert st["rounds"] * 2 < searches and st["rounds"] >= 4 * len(names)


def _small_cbs_names(bench_instances, oracle_expected):
    return [n for n in sorted(bench_instances) if "8by8" in n and oracle_expected[n]["cbs"]["rc"] == 1
            and oracle_expected[n]["cbs"]["ll"] < 60000]


def _solver(n_threads, monkeypatch):
    """A solver of its own (the engines' path stores and the worker count are fixed per solver); five threads share two
    engines, as in test_co_workers_share_an_engine."""
    from libmultirobotplanning_amd import hl
    if n_threads == 5:
        monkeypatch.setenv("MRP_HL_MAX_ENGINES", "2")
    return hl.BatchSolver(device=0, n_threads=n_threads, _lib_path=os.path.join(BUILD, "libmrp_hl_cpu.so"))


# Branches of the session driver that the mock's defaults never take: a full job ring (mrp_ll_submit answers
# MRP_LL_E_BUSY), an engine that rejects root chains, the static split, admission control, no root fast path, a shallow
# device queue with scrambled completions, and the rounds schedule.  (environment, mode)
SCHEDULE_BRANCHES = {
    "busy1": ({"MRP_MOCK_BUSY": "1"}, 0),
    "busy3_store": ({"MRP_MOCK_BUSY": "3", "MRP_MOCK_PATH_STORE": "1"}, 0),
    "chain_reject_store": ({"MRP_MOCK_CHAIN_REJECT": "1", "MRP_MOCK_PATH_STORE": "1"}, 0),
    "static_split": ({"MRP_HL_STATIC_SPLIT": "1"}, 0),
    "static_split_limit2_store": ({"MRP_HL_STATIC_SPLIT": "1", "MRP_HL_ACTIVE_LIMIT": "2", "MRP_MOCK_PATH_STORE": "1"}, 0),
    "no_root_fast_store": ({"MRP_HL_ROOT_FAST": "0", "MRP_MOCK_PATH_STORE": "1"}, 0),
    "ring2_limit3_shuffle5": ({"MRP_HL_RING_DEPTH": "2", "MRP_HL_ACTIVE_LIMIT": "3", "MRP_MOCK_SHUFFLE": "5"}, 0),
    "rounds_mode": ({}, 1),
}


@pytest.mark.parametrize("n_threads", [1, 2, 5])
@pytest.mark.parametrize("branch", sorted(SCHEDULE_BRANCHES))
def test_schedule_branches_give_the_oracles_results(cpu_solver, bench_instances, oracle_expected, monkeypatch, branch,
                                                    n_threads):
    from libmultirobotplanning_amd import hl
    env, mode = SCHEDULE_BRANCHES[branch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = _solver(n_threads, monkeypatch)
    try:
        for algo, key, names in ((hl.ECBS, "ecbs_w1.3", ROOT_CHAIN_NAMES),
                                 (hl.CBS, "cbs", _small_cbs_names(bench_instances, oracle_expected))):
            res, st = s.solve([bench_instances[n] for n in names], algo=algo, w=1.3, mode=mode)
            for n, r in zip(names, res):
                e = oracle_expected[n][key]
                assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"], _digest(r["paths"])) == (
                    hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"], e["digest"]), (n, branch, n_threads)
            if algo == hl.ECBS and branch in ("chain_reject_store", "no_root_fast_store"):
                assert st["root_solved"] == 0
            if algo == hl.ECBS and branch == "chain_reject_store":
                # no chain ran: every ticket carries one root search or the two children of a node, and every instance
                # had at most one chain rejected (a ticket without a search) — with chains, rounds * 3 < searches
                assert st["ll_searches"] / 2 <= st["rounds"] <= st["ll_searches"] + len(names)
                assert st["rounds"] >= sum(len(bench_instances[n]["starts"]) for n in names)
    finally:
        s.close()


# One engine, one worker, a synchronous mock: the run is deterministic, and the ORDER in which the driver publishes its
# searches (MRP_MOCK_TRACE: one digest per submission) is pinned together with the schedule's statistics.  Recorded from
# the driver before it was split into SessionWorker (ct_session.hpp); a change of the publication order, the backlog
# priority, admission or the chain decisions changes them.
#   (rounds, ll_searches, speculative_searches, wasted_ll_expansions, root_solved), sha256 of the trace file
SCHEDULE_TRACES = {
    "ecbs_store": ("ecbs", {"MRP_MOCK_PATH_STORE": "1"}, (37, 232, 16, 15572, 11),
                   "3fb5f1c73ad1dc840efdbbc37aa23553a3fd85878c560e22084adf6040a2e090"),
    "ecbs_store_break150": ("ecbs", {"MRP_MOCK_PATH_STORE": "1", "MRP_MOCK_CHAIN_BREAK": "150"}, (97, 232, 16, 15572, 1),
                            "1793161edebd7175e3a7b8338f1beade58b427837dd3482ba076d1e40062d51a"),
    "ecbs_tables_ring4_limit3": ("ecbs", {"MRP_HL_RING_DEPTH": "4", "MRP_HL_ACTIVE_LIMIT": "3"}, (211, 232, 16, 15572, 0),
                                 "04c8e02b7f8ac1b8b4878e5acb2a524be1d67d0386d20200f2ad8156f2f38bce"),
    "cbs": ("cbs", {}, (4691, 9532, 8382, 825, 0), "c5c917fc120238068d5c3d9dbc92c4547d3b529b2c30ac5a6efcb26c9717cc34"),
}


@pytest.mark.parametrize("config", sorted(SCHEDULE_TRACES))
def test_publication_order_is_unchanged(cpu_solver, bench_instances, oracle_expected, monkeypatch, tmp_path, config):
    from libmultirobotplanning_amd import hl
    which, env, want_stats, want_trace = SCHEDULE_TRACES[config]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    trace = tmp_path / "trace.txt"
    monkeypatch.setenv("MRP_MOCK_TRACE", str(trace))
    names = ROOT_CHAIN_NAMES if which == "ecbs" else _small_cbs_names(bench_instances, oracle_expected)
    s = _solver(1, monkeypatch)
    try:
        _, st = s.solve([bench_instances[n] for n in names], algo=hl.ECBS if which == "ecbs" else hl.CBS, w=1.3)
    finally:
        s.close()
    got = tuple(st[k] for k in ("rounds", "ll_searches", "speculative_searches", "wasted_ll_expansions", "root_solved"))
    sha = hashlib.sha256(trace.read_bytes()).hexdigest()
    print(config, got, sha)
    assert got == want_stats
    assert sha == want_trace


# ---- the prioritized-SIPP drivers (csrc/hl/sipp_drivers.hpp) against oracle.prioritized_sipp ----------------------------
# The stand-in answers an MRP_LL_SIPP job with the oracle's single-agent SIPP search, in both job forms (collision arrays;
# an engine-side table with sipp_commit), so the drivers' own part — the order of the agents, the interval bookkeeping,
# the per-instance stop, the statistics — is what is compared.
SIPP_SCHEDULES = {"session": {}, "batch": {"MRP_HL_SIPP_BATCH": "1"}}


@pytest.fixture(scope="module")
def sipp_instances(ref_tests):
    """The reference's own prioritized-SIPP fixtures and a few generated instances of 8-12 agents on small grids."""
    from libmultirobotplanning_amd import hl
    insts = [ref_tests["mapf"][n] for n in ref_tests["prioritized_sipp"]["cost"]]
    insts += [hl.generate_instance(8800 + k, 8, 8, 12, 8 + k % 5) for k in range(6)]
    insts += [hl.generate_instance(16600 + k, 16, 16, 25, 12 - k % 5) for k in range(5)]
    return insts


@pytest.fixture(scope="module")
def sipp_expected(oracle_mod, sipp_instances):
    """Per instance: oracle.prioritized_sipp's answer plus the expansions of every agent's search, from the same loop
    (mapf_prioritized_sipp.cpp:214-270) over the oracle's single-agent search."""
    out = []
    for inst in sipp_instances:
        o = dict(oracle_mod.prioritized_sipp(inst))
        o["agent_expanded"] = _sipp_agent_expansions(oracle_mod, inst, o)
        out.append(o)
    return out


def _sipp_agent_expansions(oracle_mod, inst, o):
    intervals, per_agent = [], []
    for a, (s, g) in enumerate(zip(inst["starts"], inst["goals"])):
        states, expanded, _, _ = oracle_mod.sipp_single_at(inst["dimx"], inst["dimy"], inst["obstacles"], s, g, intervals)
        per_agent.append(expanded)
        assert states == o["schedules"][a]
        first = 0
        for k in range(1, len(states) + 1):  # one interval per maximal stay on a cell, the last one open-ended
            if k == len(states) or states[k][:2] != states[first][:2]:
                intervals.append(states[first][:2] + [states[first][2], 2 ** 31 - 1 if k == len(states) else states[k][2] - 1])
                first = k
    assert sum(per_agent) == o["expanded"]
    return per_agent


def _assert_sipp_answers(res, stats, insts, expected):
    for i, (inst, r, o) in enumerate(zip(insts, res, expected)):
        assert (r["status"], r["cost"], r["n_planned"], r["planned"], r["expanded"]) == (
            0, o["cost"], o["n_planned"], o["planned"], o["expanded"]), i
        assert r["schedules"] == o["schedules"], i
    assert stats["rounds"] == max(len(inst["starts"]) for inst in insts)  # the longest chain of dependent searches
    assert stats["ll_searches"] == sum(len(inst["starts"]) for inst in insts)
    assert stats["ll_expansions"] == sum(o["expanded"] for o in expected)
    assert stats["solved"] == sum(1 for inst, o in zip(insts, expected) if o["n_planned"] == len(inst["starts"]))


@pytest.mark.parametrize("schedule", sorted(SIPP_SCHEDULES))
def test_prioritized_sipp_schedules_match_the_oracle(cpu_solver, ref_tests, sipp_instances, sipp_expected, monkeypatch, schedule):
    for k, v in SIPP_SCHEDULES[schedule].items():
        monkeypatch.setenv(k, v)
    res, stats = cpu_solver.prioritized_sipp(sipp_instances)
    _assert_sipp_answers(res, stats, sipp_instances, sipp_expected)
    exp = ref_tests["prioritized_sipp"]
    names = list(exp["cost"])
    assert [r["cost"] for r in res[:len(names)]] == [exp["cost"][n] for n in names]
    b = res[names.index("mapf_simple1b")]
    assert len(b["schedules"][0]) == exp["simple1b_lens"]["agent0"] and len(b["schedules"][1]) == 0


@pytest.mark.parametrize("knobs", [{"MRP_MOCK_BUSY": "1"}, {"MRP_MOCK_SHUFFLE": "3"}, {"MRP_HL_SIPP_WGS": "1", "MRP_HL_SIPP_TIMING": "1"}],
                         ids=["busy1", "shuffle3", "wgs1_timing"])
def test_prioritized_sipp_session_with_a_full_ring_and_scrambled_completions(cpu_solver, sipp_instances, sipp_expected,
                                                                             monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    res, stats = cpu_solver.prioritized_sipp(sipp_instances)
    _assert_sipp_answers(res, stats, sipp_instances, sipp_expected)


def test_prioritized_sipp_batch_schedule_in_two_halves(oracle_mod, cpu_solver, monkeypatch):
    """MRP_HL_SIPP_BATCH with two tickets per engine and at least 64 instances on it: the instances go in two halves that
    take turns (runSippGroup)."""
    from libmultirobotplanning_amd import hl
    insts = [hl.generate_instance(6400 + k, 8, 8, 12, 8 + k % 3) for k in range(64)]
    expected = [oracle_mod.prioritized_sipp(inst) for inst in insts]
    monkeypatch.setenv("MRP_HL_TICKETS", "2")
    monkeypatch.setenv("MRP_HL_SIPP_BATCH", "1")
    s = hl.BatchSolver(device=0, n_threads=1, _lib_path=os.path.join(BUILD, "libmrp_hl_cpu.so"))
    try:
        res, stats = s.prioritized_sipp(insts)
    finally:
        s.close()
    _assert_sipp_answers(res, stats, insts, expected)


@pytest.mark.parametrize("schedule", sorted(SIPP_SCHEDULES))
def test_prioritized_sipp_capacity_status_is_per_instance_on_the_mock(cpu_solver, sipp_instances, sipp_expected, monkeypatch,
                                                                      schedule):
    """test_hl_parity_gpu.py's test of the same name, on the CPU: a search that hits the expansion cap stops ITS instance —
    status says which, the agents planned before it keep the reference's schedules — and no other.  The cap comes from the
    oracle's own per-search expansion counts, so that some instances stop and others do not."""
    from libmultirobotplanning_amd import ll
    largest = sorted(max(o["agent_expanded"]) for o in sipp_expected)
    cap = largest[len(largest) // 2]
    assert 0 < cap and largest[0] <= cap < largest[-1]
    for k, v in SIPP_SCHEDULES[schedule].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MRP_HL_SIPP_MAX_EXPANSIONS", str(cap))
    res, _ = cpu_solver.prioritized_sipp(sipp_instances)
    stopped = 0
    for i, (r, o) in enumerate(zip(res, sipp_expected)):
        first_capped = next((a for a, e in enumerate(o["agent_expanded"]) if e > cap), None)
        if r["status"] == 0:
            assert first_capped is None, i
            assert (r["cost"], r["planned"], r["schedules"]) == (o["cost"], o["planned"], o["schedules"]), i
            continue
        stopped += 1
        assert r["status"] == ll.CAP_EXPANSIONS
        # the prefix planned before the capped search — the first one the oracle needed more than `cap` expansions for — is
        # the reference's; nothing is planned from it on
        k = first_capped
        assert k is not None, i
        assert r["planned"][:k] == o["planned"][:k] and r["planned"][k:] == [0] * (len(r["planned"]) - k)
        assert r["schedules"][:k] == o["schedules"][:k] and r["schedules"][k:] == [[]] * (len(r["planned"]) - k)
        assert r["n_planned"] == sum(o["planned"][:k])
    assert 0 < stopped < len(sipp_instances)
