"""MRP_LL_JOB_TABLE_H without a device: the truth the device tests compare with (tests/support/table_h_check.cpp over the
cases of tests/table_h_cases.py) — that it says what the cases are built for, and that its stand-alone form runs clean under
the host sanitizers and agrees with the library form —, the packer (tests/support/table_h_pack_check.cpp, a program of its
own under the sanitizers), and the Python job's flag."""
import os
import subprocess

import table_h_cases
import table_h_checker as checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _by_name():
    return {(c["name"], algo): (c, o) for algo, c, o in table_h_cases.runs()}


def test_the_cases_are_what_they_are_built_for(oracle_mod):
    runs = _by_name()
    assert len(runs) == 19
    for (name, algo), (c, o) in runs.items():
        assert o["rc"] == 0, name
        if name == "unreachable":
            assert (o["success"], o["expanded"], o["states"]) == (False, 0, []), name
            continue
        assert o["success"], name
        h0 = int(c["table"][c["start"][1], c["start"][0]])
        assert o["fmin"] >= h0 and o["cost"] >= h0, name
        assert 10 <= o["expanded"] <= 5000, (name, algo, o["expanded"])  # a few dozen to a few thousand expansions
        assert o["states"][0] == [0] + c["start"] and o["states"][-1][1:] == c["goal"], name
    # wall: the Manhattan search and the table search agree on the cost and differ in `expanded`
    for algo in (0, 1):
        c, o = runs[("wall", algo)]
        man = oracle_mod.ll_search(algo, c["map"], 0, c["start"], c["goal"], w=c["w"])
        assert man["success"] and man["cost"] == o["cost"] == 17
        assert o["expanded"] < man["expanded"], (algo, o["expanded"], man["expanded"])
    # goal_constraints: the last constraint on the goal cell is at t = 19, so the search ends at t >= 20
    assert runs[("goal_constraints", 0)][1]["cost"] >= 20
    # the focal context changes the A*-epsilon path or at least its expansion order, never A*'s answer
    assert runs[("focal", 0)][1] == runs[("wall", 0)][1]
    assert runs[("focal", 1)][1] != runs[("wall", 1)][1]
    ctx = runs[("focal_wide", 1)][0]["ctx"]
    assert ((len(ctx) + 15) // 16 * 16, max(len(p) for p in ctx)) == (32, 64)
    # the serpentine's limits: h0 beyond the narrow tier's f field; f = 125 at t <= 5; a path longer than the tier's time steps
    c, o = runs[("h0_over", 0)]
    assert int(c["table"][0, 0]) == 134 and o["cost"] == 134
    c, o = runs[("f_over", 0)]
    assert int(c["table"][c["start"][1], c["start"][0]]) == 120 and o["cost"] == 126 and o["fmin"] == 126
    assert [s[1:] for s in o["states"][:6]].count(c["start"]) >= 2  # it waited (or came back) in front of the blocked cell
    c, o = runs[("horizon", 1)]
    assert int(c["table"][c["start"][1], c["start"][0]]) == 70 and o["cost"] == 70
    c, o = runs[("big", 0)]
    assert (c["map"]["dimx"], c["map"]["dimy"]) == (48, 48) and o["cost"] >= 48
    # initial_cost: a_star.hpp:63-64,78 — cost and fmin come back offset by it
    assert runs[("initial_cost", 0)][1]["cost"] == 17 + 7 and runs[("initial_cost", 0)][1]["fmin"] == 17 + 7
    assert runs[("initial_cost", 0)][1]["states"][1:] != [] and runs[("initial_cost", 0)][1]["actions"] == runs[("wall", 0)][1]["actions"]


def test_with_the_manhattan_table_the_checker_is_the_oracle(oracle_mod):
    """The adapter replaces admissibleHeuristic and nothing else: fed the Manhattan distances as its table, it returns the
    Manhattan oracle's answer in every field."""
    import numpy as np
    for algo, c, _ in table_h_cases.runs():
        if c["name"] in ("unreachable", "big"):
            continue
        m, g = c["map"], c["goal"]
        man = np.array([[abs(x - g[0]) + abs(y - g[1]) for x in range(m["dimx"])] for y in range(m["dimy"])], dtype=np.int32)
        ctx = c["ctx"] if algo == 1 else ()
        init = c["initial_cost"] if algo == 0 else 0
        a = checker.ll_search(algo, m, c["start"], g, man, c["vc"], c["ec"], w=c["w"], agent_idx=c["agent"], ctx_paths=ctx,
                              cap_expansions=20000, initial_cost=init)
        b = oracle_mod.ll_search(algo, m, c["agent"], c["start"], g, c["vc"], c["ec"], ctx, w=c["w"], cap_expansions=20000,
                                 initial_cost=init)
        assert a == b, (c["name"], algo)


def test_the_checker_as_a_program_of_its_own_under_the_sanitizers(tmp_path):
    runs = table_h_cases.runs()
    path = tmp_path / "cases.txt"
    path.write_text(checker.case_file_text([(algo, c) for algo, c, _ in runs]))
    run = subprocess.run([checker.sanitized_program(), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(runs)
    for line, (algo, c, o) in zip(lines, runs):
        assert checker.parse_program_line(line) == o, (c["name"], algo)


def test_table_h_in_the_packer():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "table_h_pack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + ["-o", exe, os.path.join(SUPPORT, "table_h_pack_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "table_h_pack_check: ok" in run.stdout


def test_the_python_job_carries_the_flag():
    from libmultirobotplanning_amd import ll
    assert ll.JOB_TABLE_H == 256
    j = ll.LLJob(map_id=0, algo=ll.ASTAR, start=[0, 0], goal=[1, 1], table_h=True, heuristic_id=3)
    assert j.table_h and j.heuristic_id == 3 and not ll.LLJob(map_id=0, algo=ll.ASTAR, start=[0, 0], goal=[1, 1]).table_h
    with open(os.path.join(ROOT, "include", "mrp_ll.h")) as f:
        assert "#define MRP_LL_JOB_TABLE_H 256" in f.read()


def test_the_driver_tests_instances_are_solved_by_the_manhattan_oracle(oracle_mod):
    insts = table_h_cases.driver_instances()
    assert len(insts) == 16 and sorted({len(i["starts"]) for i in insts}) == [4, 5, 6]
    assert all((i["dimx"], i["dimy"], len(i["obstacles"])) == (8, 8, 12) for i in insts)
    for inst in insts:
        for algo, w in ((0, 1.0), (1, 1.3)):
            r = oracle_mod.mapf_solve(algo, inst, w=w, cap_total=table_h_cases.DRIVER_CAP)
            assert r["rc"] == 1, (inst["starts"], algo)
