"""The expansion's two short cuts — the erase at the root and the grid of focal counts (ll_compact.h compactSearch) — on the
CPU emulator: tests/support/emu_expansion.cpp is emu_ll.cpp's one-search driver with the tier's counting hook defined, built
twice, as the tier is and with -DMRP_CT_PLAIN_EXPANSION (every erase scans and bubbles, every table takes the loop over the
successors).

Both builds run the cases of tests/expansion_cases.py and every low-level call of five golden conflict trees in the three forms
of the tier (bitmap in LDS, bitmap in memory, wide): every output word equal, equal to the oracle, no access outside the window.
The counters say that the short cuts ran where they should: the grid on the sixteen-column tables and the loop on the wider
ones, no group read for an erase at the root, and erases at the root in more than a quarter of the ten-agent trees' expansions
(0.48 on 2048 synthetic ten-agent instances; a condition that the short cut is worth its test, not a target)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import expansion_cases as ex
import test_compact_emu as ce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_OK = 0
FORMS = {"bitmap_in_lds": (False, False), "bitmap_in_memory": (True, False), "wide": (True, True)}  # (bitmap in memory, wide)
ROOT_ERASES, GROUP_READS, GRID, LOOP, ERASE_FROM_256, ERASE_LAST, ROOT_ERASE_ABOVE_512 = range(7)


def _lib(plain):
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    lib = os.path.join(build, "libemu_expansion%s.so" % ("_plain" if plain else ""))
    sup, csrc = os.path.join(ROOT, "tests", "support"), os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [os.path.join(sup, "emu_expansion.cpp"), os.path.join(sup, "emu_ll.cpp"), os.path.join(sup, "wave_emu.h"),
            os.path.join(csrc, "ll_compact.h"), os.path.join(csrc, "host", "ll_pack.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fPIC", "-shared", "-Wall"] +
                              (["-DMRP_CT_PLAIN_EXPANSION"] if plain else []) + ["-o", lib, deps[0]])
    L = ctypes.CDLL(lib)
    L.emu_compact_search.restype = ctypes.c_int
    L.emu_compact_search.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ce.I32P, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ce.I32P, ctypes.c_int, ce.I32P,
                                     ctypes.c_int, ctypes.c_int, ce.I32P, ce.I32P, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ce.I64P, ce.I32P, ctypes.c_int]
    L.emu_expansion_counts.restype = None
    L.emu_expansion_counts.argtypes = [ce.I64P, ctypes.c_int]
    return L


def _counts(L):
    out = np.zeros(8, dtype=np.int64)
    L.emu_expansion_counts(out.ctypes.data_as(ce.I64P), 1)
    return [int(v) for v in out]


@pytest.fixture(scope="module")
def libs(oracle_mod):
    return _lib(False), _lib(True)


def _search(L, form, inst, agent, vc, ec, ctx_paths):
    L._bg, L._wide = FORMS[form]
    _counts(L)
    r = ce.emu_search(L, True, inst, agent, inst["starts"][agent], inst["goals"][agent], vc, ec, ctx_paths, ex.W,
                      lds_path_bytes=0)  # no room in the window: the table is read from memory
    return r, _counts(L)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ex.NAMES)
def test_case_equals_the_plain_build_and_the_oracle(libs, name, form):
    c = ex.case(name)
    (r, n), (rp, npl) = (_search(L, form, c["inst"], c["agent"], c["vc"], c["ec"], c["ctx_paths"]) for L in libs)
    want = ex.expected(c)
    print(name, form, {k: r[k] for k in ("status", "cost", "fmin", "n_states", "expanded")}, "counters", n[:7], "plain", npl[:7])
    assert r == rp                                   # every output word, the stray accesses among them
    assert (r["oob_reads"], r["oob_writes"]) == (0, 0)
    assert r["status"] == C_OK                       # (a search of the tier: not handed over)
    assert {k: r[k] for k in ("status", "cost", "fmin", "n_states", "expanded")} == {k: want[k] for k in ("status", "cost", "fmin", "n_states", "expanded")}
    assert r["states"] == [s[1:] for s in want["states"]]
    # what ran: the plain build never cuts short; this one takes the grid up to sixteen columns and the loop beyond
    assert (npl[ROOT_ERASES], npl[GRID]) == (0, 0)
    erases = r["expanded"] - 1                       # (the goal's pop erases nothing)
    assert n[ROOT_ERASES] >= 1 and npl[GROUP_READS] >= erases
    assert n[GROUP_READS] <= npl[GROUP_READS] - n[ROOT_ERASES]  # an erase at the root reads no group
    if name in ex.GRID:
        assert n[GRID] > 0 and n[LOOP] == 0 and npl[LOOP] == n[GRID]
    if name in ex.LOOP:
        assert n[LOOP] > 0 and n[GRID] == 0 and npl[LOOP] == n[LOOP]
    if name == "corridor":
        assert (r["expanded"], n[ROOT_ERASES], n[GROUP_READS], n[GRID] + n[LOOP]) == (5, 4, 0, 0)
    if name == "open512" and form != "wide":  # (the wide scan leaves at the hit: the group reads say less there)
        assert n[ROOT_ERASE_ABOVE_512] > 0 and n[ERASE_FROM_256] > 0
        assert npl[GROUP_READS] - n[GROUP_READS] >= 3 * n[ROOT_ERASE_ABOVE_512]  # three groups skipped by each of those
    if name == "erase_last":
        assert n[ERASE_LAST] > 0 and n[ERASE_LAST] == npl[ERASE_LAST]


def test_the_wide_table_gives_the_search_of_the_narrow_one():
    for a in ("a0", "a8"):
        n16, n32 = ex.expected(ex.case("five_" + a)), ex.expected(ex.case("five32_" + a))
        assert n16 == n32
        # the counts decide: the straight ways cost 8, the search steps Left first, away from the goal, and arrives after 10
        assert (n16["cost"], n16["fmin"], n16["states"][1][1:]) == (10, 8, [9, 10])


def test_golden_trees_equal_the_plain_build_and_the_oracle(libs, oracle_mod, bench_instances):
    """Every low-level call of the golden agents10_ex{1,5,9,13} and agents50_ex3 trees through both builds, three forms each."""
    L, P = libs
    searches = 0
    ten = np.zeros(8, dtype=np.int64)
    ten_expanded = 0
    for name in ["map_32by32_obst204_agents10_ex%d" % k for k in (1, 5, 9, 13)] + ["map_32by32_obst204_agents50_ex3"]:
        inst = bench_instances[name]
        _, calls = oracle_mod.mapf_record(oracle_mod.ECBS, inst, w=ex.W)
        for form in FORMS:
            for c in calls:
                args = (form, inst, c["agent"], c["vertex_constraints"], c["edge_constraints"], c["ctx_paths"])
                (r, n), (rp, npl) = _search(L, *args), _search(P, *args)
                assert r == rp, (name, form, c["agent"])
                assert (r["oob_reads"], r["oob_writes"]) == (0, 0)
                assert (npl[ROOT_ERASES], npl[GRID]) == (0, 0)
                if r["status"] == -1:  # handed over: the arena tier's
                    continue
                searches += 1
                assert (r["status"] == 0, r["expanded"]) == (c["success"], c["expanded"]), (name, form, c["agent"])
                if c["success"]:
                    assert (r["cost"], r["fmin"], r["states"]) == (c["cost"], c["fmin"], c["states"]), (name, form, c["agent"])
                wide_table = "agents50" in name
                assert n[LOOP if not wide_table else GRID] == 0, (name, form)
                if not wide_table and form == "bitmap_in_memory":
                    ten += np.asarray(n, dtype=np.int64)
                    ten_expanded += r["expanded"]
    share = ten[ROOT_ERASES] / ten_expanded
    print("%d searches; ten-agent trees, bitmap in memory: %d expansions, %d erases at the root (%.3f), %d group reads, %d grids"
          % (searches, ten_expanded, ten[ROOT_ERASES], share, ten[GROUP_READS], ten[GRID]))
    assert searches >= 200
    assert share > 0.25
