"""The select-address stores of the expansion's heap steps and the straight-line top of the search loop (ll_compact.h
ldsStoreSel, compactSearch's one sign test for all of its exits) on the CPU emulator: tests/support/emu_select.cpp is
emu_ll.cpp's one-search driver with the tier's counting hook (the loop's exits among the counters) and the hook at the end of
a search, which keeps the LDS window as the search left it.  Built as the tier is, with -DMRP_CT_EXEC_STORES (the masked
stores), with -DMRP_CT_PLAIN_LOOP (the loop top that tests the goal twice and the limits one by one), with both and with
-DMRP_CT_PLAIN_EXPANSION (every short cut off) — each with four and with three 256-entry groups in the narrow tier.

Every build runs the cases of tests/loop_exit_cases.py, tests/push_cases.py (tests/expansion_cases.py's among them), every
low-level call of five golden conflict trees and the golden jobs in the three forms of the tier (bitmap in LDS, bitmap in
memory, wide), and the task-assignment search: every output word equal across the builds and equal to the oracle's, no access
outside the window, and the window after each search equal word for word across the builds but for the scratch word.  The
counters say that the searches went where they should; each class must be met, none is a target."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import loop_exit_cases as lx
import push_cases as pc
import test_compact_emu as ce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"bitmap_in_lds": (False, False), "bitmap_in_memory": (True, False), "wide": (True, True)}  # (bitmap in memory, wide)
VARIANTS = {"product": [], "exec_stores": ["-DMRP_CT_EXEC_STORES"], "plain_loop": ["-DMRP_CT_PLAIN_LOOP"],
            "exec_stores_plain_loop": ["-DMRP_CT_EXEC_STORES", "-DMRP_CT_PLAIN_LOOP"], "plain": ["-DMRP_CT_PLAIN_EXPANSION"]}
GROUPS = (4, 3)
SLOTS = 48
U8P = ctypes.POINTER(ctypes.c_uint8)
OUT = ("status", "cost", "fmin", "n_states", "expanded")
# counters of emu_select.cpp (0 .. 30: emu_push.cpp's)
CLASSES = dict(root_erases=0, erase_of_the_last_element=5, bubbled=7, deeper_open=22, deeper_focal=23, push_into_position_0=24,
               goal_pops=31, start_is_goal=32, open_list_ran_empty=33, goal_cell_too_early=34, expansion_cap=35,
               overflow_open=36, overflow_t=37, overflow_focal_field=38, pop_empties_a_list=40, idle_side_beyond_31=41,
               idle_side_beyond_63=42, heap_crossing_32_or_64=43, one_open_push_no_focal_push=44)


def _lib(variant, groups):
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    lib = os.path.join(build, "libemu_select_%s_g%d.so" % (variant, groups))
    sup, csrc = os.path.join(ROOT, "tests", "support"), os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [os.path.join(sup, "emu_select.cpp"), os.path.join(sup, "emu_ll.cpp"), os.path.join(sup, "wave_emu.h"),
            os.path.join(csrc, "ll_compact.h"), os.path.join(csrc, "host", "ll_pack.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                               "-DMRP_CT_NARROW_GROUPS=%d" % groups] + VARIANTS[variant] + ["-o", lib, deps[0]])
    L = ctypes.CDLL(lib)
    L.emu_compact_search.restype = ctypes.c_int
    L.emu_compact_search.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ce.I32P, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ce.I32P, ctypes.c_int, ce.I32P,
                                     ctypes.c_int, ctypes.c_int, ce.I32P, ce.I32P, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ce.I64P, ce.I32P, ctypes.c_int]
    L.emu_compact_search_ta.restype = ctypes.c_int
    L.emu_compact_search_ta.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ce.I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, ce.I32P, ctypes.c_int, ce.I32P, ctypes.c_int, ce.I32P,
                                        ctypes.c_int64, ctypes.c_int, ctypes.c_int, ce.I64P, ce.I32P, ctypes.c_int]
    L.emu_select_counts.restype = None
    L.emu_select_counts.argtypes = [ce.I64P, ctypes.c_int]
    L.emu_select_window.restype = ctypes.c_int
    L.emu_select_window.argtypes = [U8P, ctypes.c_int]
    L.emu_select_scratch_offset.restype = ctypes.c_int
    return L


def _counts(L):
    out = np.zeros(SLOTS, dtype=np.int64)
    L.emu_select_counts(out.ctypes.data_as(ce.I64P), 1)
    return out


def _window(L):
    """The window of the last search as words, the scratch word zeroed (nothing reads it; it is what the last lane that was
    off has stored, or — with the masked stores — the garbage of the job before), and the job block, which the search only
    reads."""
    n = L.emu_select_window(None, 0)
    buf = np.zeros(n, dtype=np.uint8)
    assert L.emu_select_window(buf.ctypes.data_as(U8P), n) == n and n % 4 == 0
    w = buf.view(np.uint32).copy()
    w[L.emu_select_scratch_offset() // 4] = 0
    w[256 // 4:384 // 4] = 0  # (the CJob block: the job's own words, host pointers among them)
    return w


@pytest.fixture(scope="module", params=GROUPS, ids=["groups4", "groups3"])
def libs(request, oracle_mod):
    return {v: _lib(v, request.param) for v in VARIANTS}


@pytest.fixture(scope="module")
def seen():
    """The product's counters over everything this module ran (the last test reads them)."""
    return np.zeros(SLOTS, dtype=np.int64)


def _all_builds(libs, seen, form, eps, inst, agent, vc, ec, ctx_paths, w, what, **knobs):
    """One search through the five builds: equal output words, equal windows, no stray access.  Returns the product's."""
    got = {}
    for v, L in libs.items():
        L._bg, L._wide = FORMS[form]
        _counts(L)
        r = ce.emu_search(L, eps, inst, agent, inst["starts"][agent], inst["goals"][agent], vc, ec, ctx_paths, w,
                          lds_path_bytes=0, **knobs)  # no room in the window: the table is read from memory
        got[v] = (r, _counts(L), _window(L) if r.get("nodes") is not None else None)
    r, n, win = got["product"]
    for v, (rv, nv, wv) in got.items():
        assert rv == r, (what, form, v, rv, r)           # every output word, the stray accesses among them
        assert list(nv[31:45]) == list(n[31:45]), (what, form, v)  # the same exits, the same pops
        if win is not None:
            diff = np.nonzero(wv != win)[0]
            assert diff.size == 0, (what, form, v, "window words", diff[:8].tolist())
    assert (r["oob_reads"], r["oob_writes"]) == (0, 0), (what, form)
    seen += n
    return r, n


@pytest.mark.parametrize("name,form", [(n, f) for n in lx.NAMES for f in lx.forms_of(n)])
def test_loop_exit_case(libs, seen, name, form):
    c = lx.case(name)
    assert form in c["forms"]
    r, n = _all_builds(libs, seen, form, True, c["inst"], 0, c["vc"], c["ec"], c["ctx_paths"], lx.W, name, max_exp=c["max_exp"],
                       open_cap=c["open_cap"], max_t=c["max_t"])
    print(name, form, {k: r[k] for k in OUT}, "counters", {k: int(n[i]) for k, i in CLASSES.items() if n[i]})
    want = lx.expected(c)
    if c["kind"] == "oracle":
        assert {k: r[k] for k in OUT} == {k: want[k] for k in OUT}
        assert r["states"] == want["states"]
    elif c["kind"] == "cap":
        assert (r["status"], r["expanded"]) == (2, c["max_exp"] + 1) and n[35] == 1
    else:  # handed over: the code says why, and `expanded` counts the pops before it — fewer than the whole search has
        assert (r["status"], r["cost"]) == (-1, c["code"]) and r["expanded"] < want["expanded"] and n[35 + c["code"]] == 1
    if name == "start_is_goal":
        assert (n[31], n[32], r["expanded"]) == (1, 1, 1)
    if name == "walled_in":
        assert (n[33], r["status"], r["expanded"]) == (1, 1, 1)
    if name in ("goal_early", "cap_exact"):
        assert n[34] >= 1 and n[31] == 1 and n[35] == 0
    if name == "open_only":
        assert n[44] >= 1
    if name == "over_fh_narrow":
        assert r["expanded"] == 2                       # the pops at t = 0 and 1; the one at t = 2 holds focalH 381
    if name == "over_fh_wide":
        assert r["expanded"] == 1                       # the first expansion's successor does not fit


@pytest.mark.parametrize("form", list(FORMS))
def test_push_cases(libs, seen, form):
    for c in pc.cases():
        r, _ = _all_builds(libs, seen, form, True, c["inst"], c["agent"], c["vc"], c["ec"], c["ctx_paths"], pc.W, c["name"])
        want = pc.expected(c)
        assert {k: r[k] for k in OUT} == {k: want[k] for k in OUT}, c["name"]
        assert r["states"] == [s[1:] for s in want["states"]], c["name"]


def test_golden_trees(libs, seen, oracle_mod, bench_instances):
    """Every low-level call of the golden agents10_ex{1,5,9,13} and agents50_ex3 trees through the five builds, three forms."""
    searches = 0
    for name in ["map_32by32_obst204_agents10_ex%d" % k for k in (1, 5, 9, 13)] + ["map_32by32_obst204_agents50_ex3"]:
        inst = bench_instances[name]
        _, calls = oracle_mod.mapf_record(oracle_mod.ECBS, inst, w=pc.W)
        for form in FORMS:
            for c in calls:
                r, _ = _all_builds(libs, seen, form, True, inst, c["agent"], c["vertex_constraints"], c["edge_constraints"],
                                   c["ctx_paths"], pc.W, (name, c["agent"]))
                if r["status"] == -1:  # handed over: the arena tier's
                    continue
                searches += 1
                assert (r["status"] == 0, r["expanded"]) == (c["success"], c["expanded"]), (name, form, c["agent"])
                if c["success"]:
                    assert (r["cost"], r["fmin"], r["states"]) == (c["cost"], c["fmin"], c["states"]), (name, form, c["agent"])
    assert searches >= 200


def test_golden_jobs(libs, seen, bench_instances, ll_jobs_golden):
    """tests/golden/ll_jobs.json (committed inputs and oracle outputs) through the five builds."""
    n = 0
    for j in ll_jobs_golden:
        inst, a, eps = bench_instances[j["instance"]], j["agent"], j["algo"] == "ecbs"
        for form in (FORMS if eps else ("bitmap_in_lds",)):
            r, _ = _all_builds(libs, seen, form, eps, inst, a, j["vertex_constraints"], j["edge_constraints"],
                               j["ctx_paths"] if eps else [], j["w"], (j["instance"], a))
            if r["status"] == -1:
                continue
            assert (r["status"] == 0, r["expanded"]) == (j["success"], j["expanded"]), (j["instance"], a, form)
            if j["success"]:
                assert (r["cost"], r["fmin"], r["states"]) == (j["cost"], j["fmin"], j["states"]), (j["instance"], a, form)
        n += 1
    assert n >= 204


def test_task_assignment_search(libs, oracle_mod, bench_instances):
    """compactSearchTA (one heap, dualSiftUp's select-address store on every push and decrease-key) through the five builds."""
    inst = bench_instances["map_8by8_obst12_agents6_ex1"]
    m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
    n = 0
    for a in range(len(inst["starts"])):
        s, g = inst["starts"][a], inst["goals"][a]
        for goal, vc in ((g, []), (g, [[9, g[0], g[1]], [2, s[0], s[1]]]), (None, [[4, s[0], s[1]]])):
            o = oracle_mod.ta_ll_search(m, s, goal, vc, [])
            got = {}
            for v, L in libs.items():
                r = ce.emu_search_ta(L, m, s, goal, vc, [])
                got[v] = (r, _window(L))
            r, win = got["product"]
            for v, (rv, wv) in got.items():
                assert rv == r and np.array_equal(wv, win), (a, goal, v)
            assert (r["oob_reads"], r["oob_writes"]) == (0, 0)
            assert ce._compare_ta(r, o), (a, goal)
            n += 1
    assert n == 3 * len(inst["starts"])


def test_every_class_was_met(libs, seen):
    """(Runs last: the product's counters over the searches above.)"""
    got = {k: int(seen[i]) for k, i in CLASSES.items()}
    print(got)
    assert [k for k, v in got.items() if v == 0] == []
