"""What a solve call asks of its engines before and around its worker threads: tier geometry, occupancy queries, store
reserves, session launches and the co-worker count, on a machine without a GPU.

The drivers are compiled against the oracle-backed stand-ins of tests/support/, whose MRP_MOCK_CALL_LOG writes one line per
such call.  The lines of one solver are grouped by engine (engines race each other in the file) and compared with a table
recorded from the driver BEFORE its launch arithmetic was taken out of mrp_hl_solver_solve_stream (csrc/hl/launch_plan.hpp):
a change of a heavy-workgroup total, the displaced-workgroup rule, a store size, a clamp or the order of the calls changes
them.  The solves only have to reach their launches (max_hl_expansions=1); nothing is asserted about the solutions.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
LIBS = {"plain": ("libmrp_hl_cpu_plan.so", "mock_ll.cpp"), "sets": ("libmrp_hl_cpu_plan_sets.so", "mock_ll_sets.cpp")}

# instances by the class of their agent count (the heavy-workgroup total depends on the LARGEST instance of a call)
A10 = ["map_32by32_obst204_agents10_ex%d" % k for k in range(8)]
A30 = A10[:7] + ["map_32by32_obst204_agents30_ex2"]
A100 = A10[:7] + ["map_32by32_obst204_agents100_ex0"]
WIDE = "4,12,12928,40000"      # MRP_MOCK_GEOMETRY: a heavy window beyond 32 KB takes room as if it had 64 KB
NO_FRONT = "4,12,65536,40000"  # ... and front windows so large that 256 heavy workgroups leave no front workgroup at all
STORE = {"MRP_MOCK_PATH_STORE": "1"}
CONS = {"MRP_HL_DEVICE_CONSTRAINTS": "1"}

# name: (algo, worker threads, MRP_HL_MAX_ENGINES, instances, environment, keywords)
#   keywords: lib ("plain" / "sets"), mode, solver (BatchSolver arguments), solves (calls on the same solver),
#   stream (engine counts the batches of ONE stream call are prepared for)
CASES = {
    "ecbs_t8_a10": ("ecbs", 8, None, A10, {}, {}),
    "ecbs_t8_a30": ("ecbs", 8, None, A30, {}, {}),
    "ecbs_t8_a100": ("ecbs", 8, None, A100, {}, {}),
    "ecbs_t1_a10": ("ecbs", 1, None, A10, {}, {}),
    "ecbs_t2_a30": ("ecbs", 2, None, A30, {}, {}),
    "ecbs_t5_e2_a10": ("ecbs", 5, 2, A10, {}, {}),
    "ecbs_t8_three_instances": ("ecbs", 8, None, A10[:3], STORE, {}),
    "cbs_t8": ("cbs", 8, None, A10, {}, {}),
    "cbs_t1": ("cbs", 1, None, A10, {}, {}),
    "cbs_t2": ("cbs", 2, None, A10, {}, {}),
    "cbs_t5_e2": ("cbs", 5, 2, A10, {}, {}),
    "ecbs_wide_heavy_window": ("ecbs", 8, None, A10, {"MRP_MOCK_GEOMETRY": WIDE}, {}),
    "ecbs_wide_heavy_window_a100": ("ecbs", 8, None, A100, {"MRP_MOCK_GEOMETRY": WIDE}, {}),
    "ecbs_no_front_left": ("ecbs", 8, None, A100, {"MRP_MOCK_GEOMETRY": NO_FRONT}, {}),
    "ecbs_small_engines": ("ecbs", 8, None, A10, {}, {"solver": {"slots": 32}}),
    "ecbs_heavy_wgs_0": ("ecbs", 8, None, A10, {"MRP_HL_HEAVY_WGS": "0"}, {}),
    "ecbs_heavy_wgs_100": ("ecbs", 8, None, A10, {"MRP_HL_HEAVY_WGS": "100"}, {}),
    "ecbs_session_wgs": ("ecbs", 8, None, A10, {"MRP_HL_SESSION_WGS": "40"}, {}),
    "ecbs_tier": ("ecbs", 8, None, A10, {"MRP_HL_TIER": "1024,32,4096"}, {}),
    "cbs_tier": ("cbs", 8, None, A10, {"MRP_HL_TIER": "1024,32,4096"}, {}),
    "ecbs_tier_malformed": ("ecbs", 2, None, A30, {"MRP_HL_TIER": "1024,32"}, {}),
    "ecbs_callers_geometry": ("ecbs", 2, None, A10, {}, {"solver": {"lds_nodes": 1024}}),
    "ecbs_no_lds_tier": ("ecbs", 2, None, A10, {}, {"solver": {"lds_nodes": -1}}),
    "ecbs_store": ("ecbs", 8, None, A10, STORE, {}),
    "ecbs_store_t2_twice": ("ecbs", 2, None, A10, STORE, {"solves": 2}),
    "ecbs_no_store_twice": ("ecbs", 2, None, A10, {}, {"solves": 2}),
    "ecbs_path_slots_0": ("ecbs", 2, None, A10, dict(STORE, MRP_HL_PATH_SLOTS="0"), {}),
    "ecbs_path_slots_5000": ("ecbs", 2, None, A10, dict(STORE, MRP_HL_PATH_SLOTS="5000"), {}),
    "ecbs_store_max_agents": ("ecbs", 2, None, A30, dict(STORE, MRP_HL_STORE_MAX_AGENTS="20"), {}),
    "ecbs_cons": ("ecbs", 8, None, A10, dict(STORE, **CONS), {"lib": "sets"}),
    "cbs_cons_twice": ("cbs", 2, None, A10, CONS, {"lib": "sets", "solves": 2}),
    "cbs_cons_sized": ("cbs", 5, 2, A10, dict(CONS, MRP_HL_CONS_SLOTS="1000", MRP_HL_CONS_WORDS="16"), {"lib": "sets"}),
    "cbs_cons_words_clamped": ("cbs", 2, None, A10, dict(CONS, MRP_HL_CONS_WORDS="5000"), {"lib": "sets"}),
    "cbs_cons_engine_without": ("cbs", 2, None, A10, CONS, {}),
    "cbs_cons_0": ("cbs", 2, None, A10, {"MRP_HL_DEVICE_CONSTRAINTS": "0"}, {"lib": "sets"}),
    "ecbs_workers_3": ("ecbs", 2, None, A10, {"MRP_HL_WORKERS": "3"}, {}),
    "ecbs_static_split": ("ecbs", 5, 2, A10, {"MRP_HL_STATIC_SPLIT": "1"}, {}),
    "ecbs_rounds_mode": ("ecbs", 8, None, A10, dict(STORE, **CONS), {"lib": "sets", "mode": 1}),
    "ecbs_stream_2_and_4_engines": ("ecbs", 8, None, A10, STORE, {"stream": (2, 4)}),
}

# name: ((engines, "call arguments; call arguments; ..."), ...) — recorded, see above
EXPECTED = {
    "cbs_cons_0": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; session_begin_tiers_gated 0 512 0 2; "
              "session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 32; session_begin_tiers_gated 0 512 0 2; session_end tags=0"),
    ),
    "cbs_cons_engine_without": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; session_begin_tiers_gated 0 512 0 2; "
              "session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 32; session_begin_tiers_gated 0 512 0 2; session_end tags=0"),
    ),
    "cbs_cons_sized": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; "
              "constraint_store_reserve 1000 16 -> 0; session_begin_tiers_gated 0 512 0 2; session_end tags=2"),
        ("1", "create; configure_tiers 2048 64 32; constraint_store_reserve 1000 16 -> 0; "
              "session_begin_tiers_gated 0 512 0 2; session_end tags=2"),
    ),
    "cbs_cons_twice": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; "
              "constraint_store_reserve 2097152 64 -> 0; session_begin_tiers_gated 0 512 0 2; "
              "session_end tags=0; configure_tiers 2048 64 32; session_occupancy 0; "
              "session_begin_tiers_gated 0 512 0 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 32; constraint_store_reserve 2097152 64 -> 0; "
              "session_begin_tiers_gated 0 512 0 2; session_end tags=0; configure_tiers 2048 64 32; "
              "session_begin_tiers_gated 0 512 0 2; session_end tags=0"),
    ),
    "cbs_cons_words_clamped": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; "
              "constraint_store_reserve 2097152 2048 -> 0; session_begin_tiers_gated 0 512 0 2; "
              "session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 32; constraint_store_reserve 2097152 2048 -> 0; "
              "session_begin_tiers_gated 0 512 0 2; session_end tags=0"),
    ),
    "cbs_t1": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; session_begin_tiers_gated 0 512 0 1; "
              "session_end tags=0"),
    ),
    "cbs_t2": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; session_begin_tiers_gated 0 512 0 2; "
              "session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 32; session_begin_tiers_gated 0 512 0 2; session_end tags=0"),
    ),
    "cbs_t5_e2": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; session_begin_tiers_gated 0 512 0 2; "
              "session_end tags=2"),
        ("1", "create; configure_tiers 2048 64 32; session_begin_tiers_gated 0 512 0 2; session_end tags=2"),
    ),
    "cbs_t8": (
        ("0", "create; configure_tiers 2048 64 32; session_occupancy 0; session_begin_tiers_gated 0 128 0 8; "
              "session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 32; session_begin_tiers_gated 0 128 0 8; session_end tags=0"),
    ),
    "cbs_tier": (
        ("0", "create; configure_tiers 1024 32 32; session_occupancy 0; session_begin_tiers_gated 0 128 0 8; "
              "session_end tags=0"),
        ("1-7", "create; configure_tiers 1024 32 32; session_begin_tiers_gated 0 128 0 8; session_end tags=0"),
    ),
    "ecbs_callers_geometry": (
        ("0", "create; session_occupancy 1; session_tiers_geometry; path_store_reserve 2097152 -> -2; "
              "path_store_reserve 0 -> -2; session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
        ("1", "create; session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
    ),
    "ecbs_cons": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> 0; constraint_store_reserve 524288 64 -> 0; "
              "session_begin_tiers_gated 1 322 20 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 2048; path_store_reserve 524288 -> 0; "
                "constraint_store_reserve 524288 64 -> 0; session_begin_tiers_gated 1 322 20 8; "
                "session_end tags=0"),
    ),
    "ecbs_heavy_wgs_0": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 128 0 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 128 0 8; session_end tags=0"),
    ),
    "ecbs_heavy_wgs_100": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 343 13 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 343 13 8; session_end tags=0"),
    ),
    "ecbs_no_front_left": (
        ("0", "create; configure_tiers 2048 64 14336; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 16 0 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 14336; session_begin_tiers_gated 1 16 0 8; session_end tags=0"),
    ),
    "ecbs_no_lds_tier": (
        ("0", "create; session_occupancy 1; path_store_reserve 2097152 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 512 0 2; session_end tags=0"),
        ("1", "create; session_begin_tiers_gated 1 512 0 2; session_end tags=0"),
    ),
    "ecbs_no_store_twice": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 2097152 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=0; configure_tiers 2048 64 2048; "
              "session_occupancy 1; session_tiers_geometry; path_store_reserve 2097152 -> -2; "
              "path_store_reserve 0 -> -2; session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 432 80 2; "
              "session_end tags=0; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 432 80 2; "
              "session_end tags=0"),
    ),
    "ecbs_path_slots_0": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
    ),
    "ecbs_path_slots_5000": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 5000 -> 0; session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 2048; path_store_reserve 5000 -> 0; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
    ),
    "ecbs_rounds_mode": (
        ("0-7", "create"),
    ),
    "ecbs_session_wgs": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 40 20 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 40 20 8; session_end tags=0"),
    ),
    "ecbs_small_engines": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 16 0 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 16 0 8; session_end tags=0"),
    ),
    "ecbs_static_split": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 2097152 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
    ),
    "ecbs_store": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> 0; session_begin_tiers_gated 1 322 20 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 2048; path_store_reserve 524288 -> 0; "
                "session_begin_tiers_gated 1 322 20 8; session_end tags=0"),
    ),
    "ecbs_store_max_agents": (
        ("0", "create; configure_tiers 2048 64 4096; session_occupancy 1; session_tiers_geometry; "
              "session_begin_tiers_gated 1 416 96 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 4096; session_begin_tiers_gated 1 416 96 2; session_end tags=0"),
    ),
    "ecbs_store_t2_twice": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 2097152 -> 0; session_begin_tiers_gated 1 432 80 2; session_end tags=0; "
              "configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 2048; path_store_reserve 2097152 -> 0; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=0; configure_tiers 2048 64 2048; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
    ),
    "ecbs_stream_2_and_4_engines": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 2097152 -> 0; session_begin_tiers_gated 1 432 80 2; session_end tags=2"),
        ("1", "create; configure_tiers 2048 64 2048; path_store_reserve 2097152 -> 0; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=2"),
        ("2-7", "create; path_store_reserve 2097152 -> 0"),
    ),
    "ecbs_t1_a10": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 4194304 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 352 160 1; session_end tags=0"),
    ),
    "ecbs_t2_a30": (
        ("0", "create; configure_tiers 2048 64 4096; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 2097152 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 416 96 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 4096; session_begin_tiers_gated 1 416 96 2; session_end tags=0"),
    ),
    "ecbs_t5_e2_a10": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 2097152 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=2"),
        ("1", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 432 80 2; session_end tags=2"),
    ),
    "ecbs_t8_a10": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 322 20 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 322 20 8; session_end tags=0"),
    ),
    "ecbs_t8_a100": (
        ("0", "create; configure_tiers 2048 64 14336; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 254 32 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 14336; session_begin_tiers_gated 1 254 32 8; session_end tags=0"),
    ),
    "ecbs_t8_a30": (
        ("0", "create; configure_tiers 2048 64 4096; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 286 24 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 4096; session_begin_tiers_gated 1 286 24 8; session_end tags=0"),
    ),
    "ecbs_t8_three_instances": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 1398101 -> 0; session_begin_tiers_gated 1 458 54 3; session_end tags=0"),
        ("1-2", "create; configure_tiers 2048 64 2048; path_store_reserve 1398101 -> 0; "
                "session_begin_tiers_gated 1 458 54 3; session_end tags=0"),
        ("3-7", "create; path_store_reserve 1398101 -> 0"),
    ),
    "ecbs_tier": (
        ("0", "create; configure_tiers 1024 32 4096; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 322 20 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 1024 32 4096; session_begin_tiers_gated 1 322 20 8; session_end tags=0"),
    ),
    "ecbs_tier_malformed": (
        ("0", "create; configure_tiers 2048 64 4096; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 2097152 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 416 96 2; session_end tags=0"),
        ("1", "create; configure_tiers 2048 64 4096; session_begin_tiers_gated 1 416 96 2; session_end tags=0"),
    ),
    "ecbs_wide_heavy_window": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 282 20 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 282 20 8; session_end tags=0"),
    ),
    "ecbs_wide_heavy_window_a100": (
        ("0", "create; configure_tiers 2048 64 14336; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 524288 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 190 32 8; session_end tags=0"),
        ("1-7", "create; configure_tiers 2048 64 14336; session_begin_tiers_gated 1 190 32 8; session_end tags=0"),
    ),
    "ecbs_workers_3": (
        ("0", "create; configure_tiers 2048 64 2048; session_occupancy 1; session_tiers_geometry; "
              "path_store_reserve 2097152 -> -2; path_store_reserve 0 -> -2; "
              "session_begin_tiers_gated 1 432 80 2; session_end tags=2"),
        ("1", "create; configure_tiers 2048 64 2048; session_begin_tiers_gated 1 432 80 2; session_end tags=0"),
    ),
}


def _lib(which):
    os.makedirs(BUILD, exist_ok=True)
    name, mock = LIBS[which]
    out = os.path.join(BUILD, name)
    srcs = [os.path.join(ROOT, "libmultirobotplanning_amd", "csrc", "hl", "mrp_hl.cpp"),
            os.path.join(ROOT, "tests", "support", mock)]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-o", out] + srcs + ["-L", os.path.join(ROOT, "oracle"), "-loracle",
                                                "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return out


@pytest.fixture(scope="module")
def plan_libs(oracle_mod):
    return {which: _lib(which) for which in LIBS}


def _ranges(engines):
    """[0, 1, 2, 5] -> "0-2,5" """
    out, k = [], 0
    while k < len(engines):
        e = k
        while e + 1 < len(engines) and engines[e + 1] == engines[e] + 1:
            e += 1
        out.append(str(engines[k]) if e == k else "%d-%d" % (engines[k], engines[e]))
        k = e + 1
    return ",".join(out)


def grouped_log(path):
    """The call log by engine, engines numbered from the solver's first; engines with the same lines share an entry."""
    per = {}
    with open(path) as f:
        for line in f:
            idx, call = line.rstrip("\n").split(" ", 1)
            per.setdefault(int(idx), []).append(call)
    first = min(per)
    by_calls = {}
    for idx in sorted(per):
        by_calls.setdefault("; ".join(per[idx]), []).append(idx - first)
    return tuple(sorted((_ranges(e), calls) for calls, e in by_calls.items()))


def run_case(name, libs, instances, log):
    """One solver, the case's solve calls, and the grouped call log they left."""
    from libmultirobotplanning_amd import hl
    which, n_threads, max_engines, names, env, kw = CASES[name]
    env = dict(env, MRP_MOCK_CALL_LOG=str(log))
    if max_engines:
        env["MRP_HL_MAX_ENGINES"] = str(max_engines)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = hl.BatchSolver(device=0, n_threads=n_threads, _lib_path=libs[kw.get("lib", "plain")], **kw.get("solver", {}))
        try:
            algo = hl.ECBS if which == "ecbs" else hl.CBS
            insts = [instances[n] for n in names]
            if "stream" in kw:
                half = len(insts) // 2
                preps = [s.prepare(part, n_threads=t, want_paths=False)
                         for part, t in zip((insts[:half], insts[half:]), kw["stream"])]
                try:
                    s.solve_stream(preps, algo=algo, w=1.3, max_hl_expansions=1)
                finally:
                    for p in preps:
                        s.release(p)
            else:
                for _ in range(kw.get("solves", 1)):
                    s.solve(insts, algo=algo, w=1.3, max_hl_expansions=1, want_paths=False, mode=kw.get("mode", 0))
        finally:
            s.close()
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return grouped_log(log)


@pytest.mark.parametrize("name", sorted(CASES))
def test_engine_calls_of_a_solve_are_unchanged(plan_libs, bench_instances, tmp_path, name):
    got = run_case(name, plan_libs, bench_instances, tmp_path / "calls.txt")
    print(name, json.dumps(got))
    assert got == EXPECTED[name]
