"""The conflict scan of a conflict-tree child without a GPU: the wave program the kernels run (csrc/ll_node_scan.h) under
the host interpretation of its vocabulary, and the ECBS session driver's MRP_HL_DEVICE_SCAN=1 path against an oracle-backed
stand-in for the engine that answers mrp_ll_submit_scan (tests/support/mock_ll_scan.cpp)."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SUPPORT = os.path.join(ROOT, "tests", "support")

from test_host_drivers_cpu import ROOT_CHAIN_NAMES

NAMES = ROOT_CHAIN_NAMES + ["map_32by32_obst204_agents50_ex0"]


def test_scan_program_on_the_emulator():
    """ll_node_scan.h against firstConflictQuadratic / countConflictsQuadratic of csrc/hl/grid_mapf.hpp: 100 000 small
    collision-rich nodes (the replaced agent at every index, its path the longest and the shortest of its node) and 200
    nodes of 65-130 agents (two and three lane chunks; the replaced agent at 0, 63, 64 and last), the table in LDS and in
    memory; no LDS access outside the window; an edge-first node and a conflict-free node must occur."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "emu_node_scan")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-pthread", "-Wall", "-Werror", "-o", exe, os.path.join(SUPPORT, "emu_node_scan.cpp")])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    # sets are the random nodes drawn, not the scans made of them: a small node of n agents is scanned 6 n times (each
    # agent as the new one; its path as drawn, the longest, the shortest; twice for the table's place), a wide one 8 times
    small, wide, scans = int(out[3].lstrip("(")), int(out[5]), int(out[7])
    assert out[0] == "ok" and small >= 100000 and wide >= 200 and scans >= 6 * small + 8 * wide


def _digest(paths):
    h = hashlib.sha256()
    for p in paths:
        h.update(("|" + ",".join("%d:%d" % (x, y) for x, y in p)).encode())
    return h.hexdigest()[:16]


def _build_driver(name, mock):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    srcs = [os.path.join(ROOT, "libmultirobotplanning_amd", "csrc", "hl", "mrp_hl.cpp"), os.path.join(SUPPORT, mock)]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-o", out] + srcs + ["-L", os.path.join(ROOT, "oracle"), "-loracle",
                                                "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return out


@pytest.fixture(scope="module")
def driver_libs(oracle_mod):
    return {"scan": _build_driver("libmrp_hl_cpu_scan.so", "mock_ll_scan.cpp"),
            "plain": _build_driver("libmrp_hl_cpu_noscan.so", "mock_ll.cpp")}


@pytest.mark.parametrize("which", ["scan", "plain"])
def test_driver_takes_conflicts_from_the_engine(driver_libs, which, bench_instances, oracle_expected, monkeypatch):
    """MRP_HL_DEVICE_SCAN=1: the children's conflicts come with their answers — the oracle's figures and schedule at
    speculation widths 1 and 4, with one worker and with co-workers — and an engine without mrp_ll_submit_scan leaves the
    driver on its own scans: same figures, device_scans == 0."""
    from libmultirobotplanning_amd import hl
    monkeypatch.setenv("MRP_MOCK_PATH_STORE", "1")
    monkeypatch.setenv("MRP_HL_DEVICE_SCAN", "1")
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
                assert (st["device_scans"] > 0) == (which == "scan"), (spec, n_threads)
        finally:
            s.close()


def test_unset_nothing_is_flagged(driver_libs, bench_instances, monkeypatch):
    """Without the variable the driver asks the engine for nothing new: no conflicts come back and none is counted."""
    from libmultirobotplanning_amd import hl
    monkeypatch.setenv("MRP_MOCK_PATH_STORE", "1")
    monkeypatch.delenv("MRP_HL_DEVICE_SCAN", raising=False)
    s = hl.BatchSolver(device=0, n_threads=1, _lib_path=driver_libs["scan"])
    try:
        _, st = s.solve([bench_instances[n] for n in NAMES[:6]], algo=hl.ECBS, w=1.3)
    finally:
        s.close()
    assert st["device_scans"] == 0
