"""The case set of tests/root_chain_cases.py on the CPU: the conditions that keep tests/test_root_chain_gpu.py from going
hollow — every root class and every hand-made edge is there, no selected search can leave the compact tier by accident, and
the model agrees with the stand-in the CPU driver tests trust (tests/support/mock_ll.cpp mockChain)."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

import root_chain_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")


@pytest.fixture(scope="module")
def cases(oracle_mod):
    return rc.select_cases()


def test_every_class_and_every_hand_made_edge_is_selected(cases):
    counts, _ = rc.survey()
    for shape, cnt in zip(rc.SHAPES, counts):
        print("%dx%d obstacles %d agents %d w %.1f: %s" % (shape[0], shape[0], shape[1], shape[2], shape[3], cnt))
    n = collections.Counter(c["cls"] for c in cases)
    parked = sum(1 for c in cases if c["parked"])
    print("selected: %d chains, %s, parked %d" % (len(cases), dict(n), parked))
    for cls in rc.CLASSES:
        assert n[cls] >= 3, (cls, n)
    assert parked >= 3, parked
    assert len(cases) <= 64 and len({c["name"] for c in cases}) == len(cases)
    by = {c["name"]: c for c in cases}
    # the hand-made edges
    assert len(by["hand/n1"]["inst"]["starts"]) == 1 and by["hand/n1"]["model"]["results"][0]["n_states"] > 1
    on_goal = by["hand/all_on_goal"]["model"]
    assert [r["n_states"] for r in on_goal["results"]] == [1, 1, 1, 1] and (on_goal["cost"], on_goal["fmin"]) == (0, -1)
    sizes = sorted(len(c["inst"]["starts"]) for c in cases if c["name"].startswith("hand/n1") and "10x10" in c["name"])
    assert sizes == [16, 17]
    assert all(c["inst"]["dimx"] == 10 for c in cases if "10x10" in c["name"])
    # every selected root is complete, and its class is what a second look at the paths says
    for c in cases:
        m = c["model"]
        assert m["n_states"] == len(c["inst"]["starts"]) and all(r["status"] == rc.OK for r in m["results"]), c["name"]
        cls, parked_again = rc.classify(m["paths"])
        assert c["parked"] == parked_again and (c["cls"] == "hand" or c["cls"] == cls), c["name"]
        assert (m["cost"] == 0) == (cls == "free") == (m["fmin"] == -1), c["name"]
    # the class the scan's ordering is tested by: at the first conflicting time step the edge pair is the smaller one, and the
    # header's order (vertex before edge) still reports the vertex pair
    for c in cases:
        if c["cls"] == "both_same_t_edge_pair_smaller":
            V, E = rc.conflicts_at(c["model"]["paths"], c["model"]["fmin"] >> 24)
            assert E[0] < V[0] and (c["model"]["fmin"] >> 16) & 0xFF == 0
            assert c["model"]["fmin"] & 0xFFFF == (V[0][0] << 8 | V[0][1]), c["name"]


def _f32_floor(w, v):
    return int(np.floor(np.float32(w) * np.float32(v)))


def test_every_selected_search_stays_inside_the_compact_tier(cases, oracle_mod):
    """The narrow tier (ll_compact.h) holds a search while: every node it expands that is no goal has t <= 61; the open list has
    five free entries of 1023 before such an expansion; focalH + 2 * n_agents_pad <= 511 at such an expansion; a path has at
    most 64 rows in the chain's focal table.  Bounds that follow from the reference's semantics (tests/limit_cases.py (E), (N)):
      time    A*-epsilon expands out of the focal list, f <= w * fmin <= w * cost, so t = g <= floor(w * cost)       <= 61
      open    an expansion pushes at most five nodes: open <= 5 * expanded + 1, + 5 free                             <= 1023
      focalH  a step adds the context agents on the new cell (vertex) and those that leave it for the old one (edge): at
              most 2 * M, M = the most context agents on one cell at one time; focalH <= 2 * M * floor(w * cost);
              + 2 * n_agents_pad                                                                                    <= 511
      states  MAX_STATES = 40, the bound the cases were selected by (expanded <= MAX_EXPANDED = 203 likewise)
    Largest values over the selected set: 17 states, floor(w * cost) = 20, 176 expansions (5 * 176 + 6 = 886), focalH bound
    (2 * M * floor(w * cost) + 2 * n_agents_pad) 120."""
    worst = dict(states=0, t=0, open=0, focal=0)
    for c in cases:
        n = len(c["inst"]["starts"])
        npad = (n + 15) & ~15
        paths = c["model"]["paths"]
        for a, r in enumerate(c["model"]["results"]):
            t_max = _f32_floor(c["w"], r["cost"])
            at = collections.Counter((t, tuple(rc.state_at(paths[b], t))) for b in range(a) for t in range(t_max + 2))
            M = max(at.values()) if at else 0
            worst = dict(states=max(worst["states"], r["n_states"]), t=max(worst["t"], t_max),
                         open=max(worst["open"], 5 * r["expanded"] + 6), focal=max(worst["focal"], 2 * M * t_max + 2 * npad))
            assert r["n_states"] <= rc.MAX_STATES and r["expanded"] <= rc.MAX_EXPANDED, (c["name"], a)
            assert t_max <= 61 and 5 * r["expanded"] + 6 <= 1023 and 2 * M * t_max + 2 * npad <= 511, (c["name"], a)
    print("largest: %s" % worst)
    # ... and the break case of the device test is what its comment says
    inst, w = rc.break_case()
    m = rc.chain_model(inst, w)
    for a, r in enumerate(m["results"]):
        assert r["status"] == rc.OK
        if a != rc.BREAK_K:
            assert _f32_floor(w, r["cost"]) + 2 < rc.BREAK_ROWS, a
    assert m["results"][rc.BREAK_K]["n_states"] > rc.BREAK_ROWS
    scan = oracle_mod.conflict_scan(m["paths"])
    assert (scan["time"], scan["agent1"], scan["agent2"], scan["type"]) == (11, rc.BREAK_K, rc.BREAK_K + 1, 0)


# ---- the model against mockChain -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mock(oracle_mod):
    """tests/support/mock_ll.cpp alone, built like the CPU driver tests' library: g++ against liboracle.so."""
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libmock_ll_chain.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "support", "mock_ll.cpp"), "-L", os.path.join(ROOT, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    from libmultirobotplanning_amd import ll
    lib = ctypes.CDLL(out)
    lib.mrp_ll_create.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.mrp_ll_destroy.argtypes = [ctypes.c_void_p]
    lib.mrp_ll_destroy.restype = None
    lib.mrp_ll_upload_map.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ll.I32P, ll.I32P]
    lib.mrp_ll_path_store_reserve.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mrp_ll_search_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ll.mrp_ll_job), ctypes.POINTER(ll.mrp_ll_result)]
    return lib


def _mock_chain(lib, h, inst, w, **kw):
    from libmultirobotplanning_amd import ll
    ob = np.ascontiguousarray(np.asarray(inst["obstacles"], dtype=np.int32).reshape(-1, 2))
    mid = ctypes.c_int32(-1)
    assert lib.mrp_ll_upload_map(h, inst["dimx"], inst["dimy"], len(ob), ob.ctypes.data_as(ll.I32P), ctypes.byref(mid)) == 0
    b = rc.Batch()
    b.add_chain(mid.value, inst, w, list(range(len(inst["starts"]))), **kw)
    b.build()
    assert lib.mrp_ll_search_batch(h, 1, b.cjobs, b.cres) == 0
    return b.result(0)


def _agree(got, model, what):
    """mockChain fills in status, cost, fmin, n_states, expanded and states (no actions)."""
    assert (got["status"], got["n_states"], got["expanded"], got["cost"], got["fmin"]) == (
        rc.OK, model["n_states"], model["expanded"], model["cost"], model["fmin"]), what
    assert len(got["chain"]) == len(model["results"]), what
    for a, (g, m) in enumerate(zip(got["chain"], model["results"])):
        assert [k for k in rc.same(g, m) if k != "actions"] == [], (what, a, g, m)


def test_the_model_agrees_with_the_mock_chain(cases, mock, monkeypatch):
    monkeypatch.setenv("MRP_MOCK_PATH_STORE", "1")
    monkeypatch.delenv("MRP_MOCK_CHAIN_BREAK", raising=False)
    monkeypatch.delenv("MRP_MOCK_CHAIN_REJECT", raising=False)
    h = ctypes.c_void_p()
    assert mock.mrp_ll_create(None, ctypes.byref(h)) == 0
    try:
        assert mock.mrp_ll_path_store_reserve(h, 32) == 0
        for c in cases:
            inst, w, whole, n = c["inst"], c["w"], c["model"], len(c["inst"]["starts"])
            _agree(_mock_chain(mock, h, inst, w), whole, c["name"])
            E = [r["expanded"] for r in whole["results"]]
            for k in sorted({1, n // 2, n - 1} - {0}):
                if k >= n:
                    continue
                # chunks: agents 0 .. k - 1, then the rest from the store the first job filled
                _agree(_mock_chain(mock, h, inst, w, count=k), rc.chain_model(inst, w, count=k), (c["name"], "count", k))
                _agree(_mock_chain(mock, h, inst, w, first=k), rc.chain_model(inst, w, first=k, prior_paths=whole["paths"]),
                       (c["name"], "first", k))
                # the shared budget runs out inside agent k's search
                budget = sum(E[:k]) + E[k] - 1
                _agree(_mock_chain(mock, h, inst, w, budget=budget), rc.chain_model(inst, w, budget=budget), (c["name"], "budget", k))
            _agree(_mock_chain(mock, h, inst, w, count=n + 3), whole, (c["name"], "count > n"))
            # MRP_MOCK_CHAIN_BREAK: a search of more than K expansions ends the chain in front of it
            K = sorted(E)[len(E) // 2]
            monkeypatch.setenv("MRP_MOCK_CHAIN_BREAK", str(K))
            _agree(_mock_chain(mock, h, inst, w), rc.chain_model(inst, w, break_before=lambda a, r: r["expanded"] > K),
                   (c["name"], "break", K))
            monkeypatch.delenv("MRP_MOCK_CHAIN_BREAK")
    finally:
        mock.mrp_ll_destroy(h)
