"""The conflict scan of a conflict-tree child from what its parent's scan established, without a GPU: the wave program
(csrc/ll_node_scan.h nodeScanFromParent) under the host interpretation of its vocabulary, the packer's handling of
MRP_LL_JOB_SCAN_FROM_PARENT, and the ECBS session driver's MRP_HL_DEVICE_SCAN_INCREMENTAL=1 path against an oracle-backed
stand-in for the engine that exports mrp_ll_submit_node and checks what the driver sends (tests/support/mock_ll_node.cpp)."""
import ctypes
import os
import subprocess

import pytest

from test_node_scan_cpu import BUILD, NAMES, ROOT, SUPPORT, _build_driver, _digest

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_from_parent_program_on_the_emulator():
    """nodeScanFromParent against firstConflictQuadratic / countConflictsQuadratic of the CHILD: small collision-rich nodes
    (every agent replaced) and nodes of 65-130 agents (the replaced agent at 0, 63, 64 and last), parent_count from
    countConflictsQuadratic of the parent, clean_before 0 / the parent's first-conflict time / T, the table in LDS and in
    memory.  The program itself insists that every case the scan distinguishes occurred (both fallback directions, count 0, a
    first conflict among other agents at or behind clean_before, one with the replaced agent before it with j < a and with
    j > a, an edge-first step, a step with both kinds, two other agents resting on one cell), feeds untruthful inputs, and
    runs under the host sanitizers with arrays of exactly the device's sizes."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "emu_node_scan_parent")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-pthread", "-Wall", "-Werror"] + SAN +
                          ["-o", exe, os.path.join(SUPPORT, "emu_node_scan_parent.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert run.returncode == 0, run.stdout
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 100000 and int(last[3]) >= 100000, run.stdout


def test_packer_takes_and_rejects_from_parent_jobs():
    """Every rejection include/mrp_ll.h lists for the flag, with no set created; an accepted job's words: no column for
    agent_idx in the focal context, the replaced path's slot and the two integers behind the ids."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "pack_node_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + ["-o", exe, os.path.join(SUPPORT, "pack_node_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "pack_node_check: ok" in run.stdout


@pytest.fixture(scope="module")
def driver_libs(oracle_mod):
    return {"node": _build_driver("libmrp_hl_cpu_node.so", "mock_ll_node.cpp"),
            "scan": _build_driver("libmrp_hl_cpu_scan_only.so", "mock_ll_scan.cpp")}


def _counts(lib_path):
    lib = ctypes.CDLL(lib_path)
    calls, flagged = ctypes.c_int64(0), ctypes.c_int64(0)
    lib.mock_ll_node_counts(ctypes.byref(calls), ctypes.byref(flagged))
    return calls.value, flagged.value


@pytest.mark.parametrize("which", ["node", "scan"])
def test_driver_scans_children_from_their_parents(driver_libs, which, bench_instances, oracle_expected, monkeypatch):
    """MRP_HL_DEVICE_SCAN_INCREMENTAL=1: the oracle's figures and schedule at speculation widths 1 and 4, with one worker and
    with co-workers; the stand-in aborts when parent_count, clean_before or the named slot are not the parent's.  An engine
    without mrp_ll_submit_node leaves the driver as with the variable unset: same figures, incremental_scans == 0."""
    from libmultirobotplanning_amd import hl
    monkeypatch.setenv("MRP_MOCK_PATH_STORE", "1")
    monkeypatch.delenv("MRP_HL_DEVICE_SCAN", raising=False)
    monkeypatch.setenv("MRP_HL_DEVICE_SCAN_INCREMENTAL", "1")
    for n_threads, engines in ((1, None), (4, "2")):
        if engines is None:
            monkeypatch.delenv("MRP_HL_MAX_ENGINES", raising=False)
        else:
            monkeypatch.setenv("MRP_HL_MAX_ENGINES", engines)
        s = hl.BatchSolver(device=0, n_threads=n_threads, _lib_path=driver_libs[which])
        try:
            for spec in (1, 4):
                monkeypatch.setenv("MRP_HL_SPEC", str(spec))
                res, st = s.solve([bench_instances[n] for n in NAMES], algo=hl.ECBS, w=1.3)
                for n, r in zip(NAMES, res):
                    e = oracle_expected[n]["ecbs_w1.3"]
                    assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"], _digest(r["paths"])) == (
                        hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"], e["digest"]), (n, spec, n_threads)
                if which == "node":
                    assert st["incremental_scans"] > 0 and st["device_scans"] >= st["incremental_scans"], (spec, n_threads)
                else:
                    assert st["incremental_scans"] == 0 and st["device_scans"] == 0, (spec, n_threads)
        finally:
            s.close()
    if which == "node":
        calls, flagged = _counts(driver_libs[which])
        assert calls > 0 and flagged > 0


def test_unset_nothing_is_flagged(driver_libs, bench_instances, monkeypatch):
    """With both variables unset the driver never calls mrp_ll_submit_node: no job is flagged, nothing is counted."""
    from libmultirobotplanning_amd import hl
    monkeypatch.setenv("MRP_MOCK_PATH_STORE", "1")
    monkeypatch.delenv("MRP_HL_DEVICE_SCAN_INCREMENTAL", raising=False)
    monkeypatch.delenv("MRP_HL_DEVICE_SCAN", raising=False)
    before = _counts(driver_libs["node"])
    s = hl.BatchSolver(device=0, n_threads=1, _lib_path=driver_libs["node"])
    try:
        _, st = s.solve([bench_instances[n] for n in NAMES], algo=hl.ECBS, w=1.3)
    finally:
        s.close()
    assert st["incremental_scans"] == 0 and st["device_scans"] == 0
    assert _counts(driver_libs["node"]) == before
