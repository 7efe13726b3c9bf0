"""The expansion's push step (ll_compact.h pushTurn: positions, stops and the elements' rows per lane) and the heap roots kept
in a register across the search loop, on the CPU emulator: tests/support/emu_push.cpp is emu_ll.cpp's one-search driver with the
tier's counting hook defined, built as the tier is (the push step on, the kept roots off: they measured slower), with
-DMRP_CT_PLAIN_EXPANSION (every short cut off), with -DMRP_CT_KEEP_TOPS (both parts on), with each part off alone
(-DMRP_CT_SCALAR_PUSHES, -DMRP_CT_LOAD_TOPS) and with -DMRP_CT_CHECK_TOPS (the kept roots, and the loop top loads the roots as
well and counts every disagreement) — and the same once more with -DMRP_CT_NARROW_GROUPS=3.

Every build runs the cases of tests/push_cases.py, every low-level call of five golden conflict trees and one CBS call set in
the three forms of the tier (bitmap in LDS, bitmap in memory, wide): every output word equal to the plain build's and to the
oracle's, no access outside the window, no disagreement of the kept roots in as many checks as there were expansions.  The
counters say that the searches went where they should; each class must be met, none is a target."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import push_cases as pc
import test_compact_emu as ce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_OK = 0
FORMS = {"bitmap_in_lds": (False, False), "bitmap_in_memory": (True, False), "wide": (True, True)}  # (bitmap in memory, wide)
# (the kept roots are off in the product, DESIGN.md section 7: -DMRP_CT_KEEP_TOPS builds them, and the checking build with them)
VARIANTS = {"product": [], "plain": ["-DMRP_CT_PLAIN_EXPANSION"], "scalar_pushes": ["-DMRP_CT_SCALAR_PUSHES"],
            "keep_tops": ["-DMRP_CT_KEEP_TOPS"], "keep_tops_scalar_pushes": ["-DMRP_CT_KEEP_TOPS", "-DMRP_CT_SCALAR_PUSHES"],
            "load_tops": ["-DMRP_CT_KEEP_TOPS", "-DMRP_CT_LOAD_TOPS"], "check_tops": ["-DMRP_CT_CHECK_TOPS"]}
GROUPS = (4, 3)
SLOTS = 32
(ROOT_ERASES, _, _, _, _, _, _, BUBBLED, CHECKS, DISAGREE, OPEN_ROOT_LAST, OPEN_ROOT_CHILD, FOCAL_ROOT_LAST, FOCAL_ROOT_CHILD, ONE,
 TWO, SUCC3, SUCC4, SUCC5, ROW2_ALONE, ROWS23, FIRST_OUT_SECOND_IN, DEEPER_OPEN, DEEPER_FOCAL, POS0, FIRST_ROOT_OPEN,
 FIRST_ROOT_FOCAL, SECOND_OVER_FIRST_OPEN, SECOND_OVER_FIRST_FOCAL, EQUAL_ROOT_OPEN, EQUAL_ROOT_FOCAL) = range(31)
CLASSES = dict(root_erases=ROOT_ERASES, bubbled=BUBBLED, open_root_last=OPEN_ROOT_LAST, open_root_child=OPEN_ROOT_CHILD,
               focal_root_last=FOCAL_ROOT_LAST, focal_root_child=FOCAL_ROOT_CHILD, one=ONE, two=TWO, succ3=SUCC3, succ4=SUCC4,
               succ5=SUCC5, row2_alone=ROW2_ALONE, rows23=ROWS23, first_out_second_in=FIRST_OUT_SECOND_IN,
               deeper_open=DEEPER_OPEN, deeper_focal=DEEPER_FOCAL, pos0=POS0, first_root_open=FIRST_ROOT_OPEN,
               first_root_focal=FIRST_ROOT_FOCAL, second_over_first_open=SECOND_OVER_FIRST_OPEN,
               second_over_first_focal=SECOND_OVER_FIRST_FOCAL, equal_root_open=EQUAL_ROOT_OPEN,
               equal_root_focal=EQUAL_ROOT_FOCAL)
OUT = ("status", "cost", "fmin", "n_states", "expanded")


def _lib(variant, groups):
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    lib = os.path.join(build, "libemu_push_%s_g%d.so" % (variant, groups))
    sup, csrc = os.path.join(ROOT, "tests", "support"), os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [os.path.join(sup, "emu_push.cpp"), os.path.join(sup, "emu_ll.cpp"), os.path.join(sup, "wave_emu.h"),
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
    L.emu_push_counts.restype = None
    L.emu_push_counts.argtypes = [ce.I64P, ctypes.c_int]
    return L


def _counts(L):
    out = np.zeros(SLOTS, dtype=np.int64)
    L.emu_push_counts(out.ctypes.data_as(ce.I64P), 1)
    return out


@pytest.fixture(scope="module", params=GROUPS, ids=["groups4", "groups3"])
def libs(request, oracle_mod):
    # (the smaller geometry: the product, the plain forms and the two builds with the kept roots)
    return {v: _lib(v, request.param) for v in VARIANTS if request.param == 4 or v in ("product", "plain", "keep_tops", "check_tops")}


@pytest.fixture(scope="module")
def seen():
    """The counters of the build with both parts on over everything this module ran (the last test reads them)."""
    return np.zeros(SLOTS, dtype=np.int64)


def _search(L, form, eps, inst, agent, vc, ec, ctx_paths, w):
    L._bg, L._wide = FORMS[form]
    _counts(L)
    r = ce.emu_search(L, eps, inst, agent, inst["starts"][agent], inst["goals"][agent], vc, ec, ctx_paths, w,
                      lds_path_bytes=0)  # no room in the window: the table is read from memory
    return r, _counts(L)


def _all_builds(libs, seen, form, eps, inst, agent, vc, ec, ctx_paths, w, what):
    """One search through the seven builds: equal output words, no stray access, the kept roots right.  Returns the product's."""
    got = {v: _search(L, form, eps, inst, agent, vc, ec, ctx_paths, w) for v, L in libs.items()}
    r, n = got["keep_tops"]  # (both parts on: its counters see the kept roots; the product's turns are compared with it below)
    for v, (rv, _) in got.items():
        assert rv == r, (what, form, v)               # every output word, the stray accesses among them
    assert (r["oob_reads"], r["oob_writes"]) == (0, 0), (what, form)
    nc = got["check_tops"][1]
    handed_over = r["status"] == -1                    # (left at a loop top: one check more than expansions)
    assert nc[DISAGREE] == 0 and nc[CHECKS] == r["expanded"] + (1 if handed_over else 0), (what, form, nc[CHECKS], nc[DISAGREE], r["expanded"])
    # what ran: the plain build neither erases at the root nor takes the new push step
    npl = got["plain"][1]
    assert (npl[ROOT_ERASES], npl[ONE] + npl[TWO]) == (0, 0)
    assert all(got[v][1][ONE] + got[v][1][TWO] == 0 for v in ("scalar_pushes", "keep_tops_scalar_pushes") if v in got)
    for v in ("product", "load_tops"):  # the same turns with the roots loaded
        if v in got:
            assert list(got[v][1][ONE:POS0 + 1]) == list(n[ONE:POS0 + 1]), (what, form, v)
    assert list(nc[:CHECKS]) + list(nc[OPEN_ROOT_LAST:SLOTS]) == list(n[:CHECKS]) + list(n[OPEN_ROOT_LAST:SLOTS]), (what, form)
    seen += n
    return r, n


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", pc.NAMES)
def test_case_equals_the_plain_build_and_the_oracle(libs, seen, name, form):
    c = pc.case(name)
    r, n = _all_builds(libs, seen, form, True, c["inst"], c["agent"], c["vc"], c["ec"], c["ctx_paths"], pc.W, name)
    want = pc.expected(c)
    print(name, form, {k: r[k] for k in OUT}, "counters", {k: int(n[i]) for k, i in CLASSES.items() if n[i]})
    assert r["status"] == C_OK                       # (a search of the tier: not handed over)
    assert {k: r[k] for k in OUT} == {k: want[k] for k in OUT}
    assert r["states"] == [s[1:] for s in want["states"]]
    if name == "corridor":                           # one successor per turn, every push into an empty list
        assert (n[ONE], n[TWO], n[FIRST_ROOT_OPEN]) == (4, 0, 4) and n[POS0] >= 4
    if name == "two_open":                           # the pair, then the pop that leaves Wait alone in the open list
        assert n[TWO] >= 1 and n[OPEN_ROOT_LAST] >= 1
    if name in ("five_a0", "five_a8"):               # the first expansion: 2 + 2 + 1, every successor within the bound
        assert n[SUCC5] >= 1 and n[ROWS23] >= 2 and n[ROW2_ALONE] >= 1


def test_golden_trees_equal_the_plain_build_and_the_oracle(libs, seen, oracle_mod, bench_instances):
    """Every low-level call of the golden agents10_ex{1,5,9,13} and agents50_ex3 trees through the five builds, three forms each."""
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
    print("%d searches" % searches)
    assert searches >= 200


def test_cbs_calls_equal_the_plain_build_and_the_oracle(libs, seen, oracle_mod, bench_instances):
    """EPS = false: the same successor loop with the focal rows idle (A* has one list; the narrow form, bitmap in LDS)."""
    searches = 0
    for name in ("map_8by8_obst12_agents6_ex1", "map_8by8_obst12_agents8_ex3", "map_8by8_obst12_agents5_ex0"):
        inst = bench_instances[name]
        _, calls = oracle_mod.mapf_record(oracle_mod.CBS, inst, w=1.0)
        for c in calls:
            r, n = _all_builds(libs, seen, "bitmap_in_lds", False, inst, c["agent"], c["vertex_constraints"], c["edge_constraints"],
                               [], 1.0, (name, c["agent"]))
            assert n[ROW2_ALONE] + n[ROWS23] == 0
            if r["status"] == -1:
                continue
            searches += 1
            assert (r["status"] == 0, r["expanded"]) == (c["success"], c["expanded"]), (name, c["agent"])
            if c["success"]:
                assert (r["cost"], r["states"]) == (c["cost"], c["states"]), (name, c["agent"])
    assert searches >= 20


def test_every_class_of_turn_push_and_pop_was_met(libs, seen):
    """(Runs last: the counters of the build with both parts on over the searches above.)"""
    got = {k: int(seen[i]) for k, i in CLASSES.items()}
    print(got)
    assert [k for k, v in got.items() if v == 0] == []
