"""ctypes binding of include/mrp_ll.h — the C-ABI of the HIP low-level search engine.

This is plumbing for tests and benchmarks; it mirrors the reference's low-level call
``LowLevelSearch_t(llenv[, w]).search(start, out)`` (cbs.hpp:99-101,155-157; ecbs.hpp:126-129,265-268) as
``LowLevelEngine.search_batch([LLJob...]) -> [LLResult...]``.  There is no CPU fallback: if the HIP library is
missing or no GPU is visible, construction raises.
"""
import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("MRP_LL_LIB") or os.path.join(_PKG, "lib", "libmrp_ll.so")

ASTAR, ASTAR_EPS, SIPP, ASTAR_TA, ASTAR_EPS_TA = 0, 1, 2, 3, 4
JOB_STORE_RESULT, JOB_NO_GOAL, JOB_ROOT_CHAIN, JOB_HEAVY = 1, 2, 4, 8  # mrp_ll_job.flags (include/mrp_ll.h)
JOB_SCAN_CONFLICTS = 16  # mrp_ll_job.flags: mrp_ll_submit_scan also returns the conflicts of the node the job completes
JOB_CONSTRAINT_SET = 32  # mrp_ll_job.flags: mrp_ll_submit_sets' sets[i] names the agent's set in the device constraint store
JOB_SCAN_FROM_PARENT = 64  # mrp_ll_job.flags: mrp_ll_submit_node's bases[i] holds what the parent node's scan established
JOB_TABLE_H = 256        # mrp_ll_job.flags: ASTAR / ASTAR_EPS take h from the shortest-path table heuristic_id (not Manhattan)
JOB_TRY_LDS = 128        # mrp_ll_job.flags: an ASTAR_EPS_TA search starts in its LDS tier (a hint; only LLResult.tier depends on it)
SCAN_UNTOUCHED = -2      # search_batch_scan: what every field of an entry the engine did not write still holds
OK, NO_SOLUTION, CAP_EXPANSIONS, CAP_NODES, CAP_HORIZON, BAD_JOB, PATH_TRUNCATED, CAP_FOCAL = range(8)
NOT_RUN = 8              # a root ended before this agent's search (mrp_ll_ta_root_batch, root chains)
E_INVALID, E_DEVICE, E_NOMEM, E_BUSY = -1, -2, -3, -4  # return codes of the API calls
ACTION_NAMES = ["Up", "Down", "Left", "Right", "Wait"]  # example/ecbs.cpp:49-55

ASSIGN_NO_EDGE = 2 ** 31 - 1  # MRP_LL_ASSIGN_NO_EDGE
ASSIGN_FREE, ASSIGN_NO_TASK, ASSIGN_SOME_TASK = -1, -2, -3  # mrp_ll_assign_problem.mode[a]; >= 0: forced to that task

I32P = ctypes.POINTER(ctypes.c_int32)
U64P = ctypes.POINTER(ctypes.c_uint64)


class mrp_ll_options(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("n_tickets", ctypes.c_int32), ("slots", ctypes.c_int32),
                ("arena_nodes", ctypes.c_int32), ("max_horizon", ctypes.c_int32), ("max_cells", ctypes.c_int32),
                ("lds_nodes", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class mrp_ll_job(ctypes.Structure):
    _fields_ = [("map_id", ctypes.c_int32), ("algo", ctypes.c_int32), ("w", ctypes.c_float),
                ("agent_idx", ctypes.c_int32), ("start_x", ctypes.c_int32), ("start_y", ctypes.c_int32),
                ("goal_x", ctypes.c_int32), ("goal_y", ctypes.c_int32),
                ("n_vertex_constraints", ctypes.c_int32), ("vertex_constraints", I32P),
                ("n_edge_constraints", ctypes.c_int32), ("edge_constraints", I32P),
                ("n_agents", ctypes.c_int32), ("path_len", I32P), ("path_xy", ctypes.POINTER(I32P)),
                ("max_expansions", ctypes.c_int64),
                ("n_collision_locations", ctypes.c_int32), ("collision_xy", I32P), ("collision_count", I32P),
                ("collision_intervals", I32P), ("initial_cost", ctypes.c_int32), ("sipp_commit", ctypes.c_int32),
                ("sipp_table", ctypes.c_void_p), ("path_ids", I32P), ("result_path_id", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("heuristic_id", ctypes.c_int32), ("chain_count", ctypes.c_int32),
                ("chain_starts_goals_xy", I32P)]


class mrp_ll_result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("cost", ctypes.c_int32), ("fmin", ctypes.c_int32),
                ("n_states", ctypes.c_int32), ("expanded", ctypes.c_int64), ("states_txy", I32P),
                ("actions", I32P), ("states_cap", ctypes.c_int32), ("tier", ctypes.c_int32),
                ("action_costs", I32P), ("chain_results", ctypes.c_void_p)]


class mrp_ll_conflict(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("found", "time", "agent1", "agent2", "type", "x1", "y1", "x2", "y2", "count")]


class mrp_ll_constraint_ref(ctypes.Structure):
    _fields_ = [("base_set_id", ctypes.c_int32), ("result_set_id", ctypes.c_int32)]


class mrp_ll_scan_base(ctypes.Structure):
    _fields_ = [("parent_count", ctypes.c_int32), ("clean_before", ctypes.c_int32)]


class mrp_ll_assign_problem(ctypes.Structure):
    _fields_ = [("n_agents", ctypes.c_int32), ("n_tasks", ctypes.c_int32), ("cost", I32P), ("heuristic_ids", I32P),
                ("starts_xy", I32P), ("allowed", U64P), ("forbidden", U64P), ("mode", I32P), ("min_matching", ctypes.c_int32)]


class mrp_ll_assign_problem_w(ctypes.Structure):  # the wide form: allowed / forbidden are [n_agents][mask_words]
    _fields_ = mrp_ll_assign_problem._fields_ + [("mask_words", ctypes.c_int32)]


class mrp_ll_assign_result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("matched", ctypes.c_int32), ("cost", ctypes.c_int64), ("task_of", I32P)]


class mrp_ll_ta_root(ctypes.Structure):
    _fields_ = [("map_id", ctypes.c_int32), ("n_agents", ctypes.c_int32), ("starts_xy", I32P), ("goals_xy", I32P),
                ("heuristic_ids", I32P), ("max_expansions", ctypes.c_int64), ("results", ctypes.POINTER(mrp_ll_result))]


class mrp_ll_stats(ctypes.Structure):
    _fields_ = [("launches", ctypes.c_int64), ("jobs", ctypes.c_int64), ("expansions", ctypes.c_int64),
                ("nodes_created", ctypes.c_int64), ("migrated", ctypes.c_int64), ("kernel_ms", ctypes.c_double),
                ("h2d_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double), ("session_busy_ms", ctypes.c_double),
                ("session_idle_ms", ctypes.c_double), ("session_active_wgs", ctypes.c_int64), ("pack_ms", ctypes.c_double),
                ("unpack_ms", ctypes.c_double), ("staged_bytes", ctypes.c_int64), ("prof", ctypes.c_int64 * 8),
                ("heavy_busy_ms", ctypes.c_double), ("heavy_idle_ms", ctypes.c_double), ("heavy_active_wgs", ctypes.c_int64),
                ("heavy_fallbacks", ctypes.c_int64)]


EXPORTS = ["mrp_ll_create", "mrp_ll_destroy", "mrp_ll_last_error", "mrp_ll_upload_map", "mrp_ll_search_batch",
           "mrp_ll_submit", "mrp_ll_wait", "mrp_ll_get_stats", "mrp_ll_reset_stats", "mrp_ll_version",
           "mrp_ll_session_begin", "mrp_ll_session_end", "mrp_ll_poll", "mrp_ll_poll_any", "mrp_ll_submit_lane", "mrp_ll_sync_maps",
           "mrp_ll_configure_tiers", "mrp_ll_session_occupancy", "mrp_ll_session_begin_sipp", "mrp_ll_release_maps", "mrp_ll_session_begin_algo", "mrp_ll_conflict_scan",
           "mrp_ll_sipp_table_create", "mrp_ll_sipp_table_add", "mrp_ll_sipp_table_destroy", "mrp_ll_path_store_reserve",
           "mrp_ll_upload_heuristic", "mrp_ll_session_begin_tiers", "mrp_ll_session_tiers_geometry",
           "mrp_ll_session_begin_tiers_gated", "mrp_ll_submit_tagged", "mrp_ll_poll_any_tagged",
           "mrp_ll_compute_heuristics", "mrp_ll_read_heuristic", "mrp_ll_heuristic_lookup", "mrp_ll_submit_scan",
           "mrp_ll_constraint_store_reserve", "mrp_ll_submit_sets", "mrp_ll_session_front_tables",
           "mrp_ll_submit_node", "mrp_ll_assign_batch", "mrp_ll_assign_series_create", "mrp_ll_assign_series_next",
           "mrp_ll_assign_series_destroy", "mrp_ll_assign_batch_w", "mrp_ll_assign_series_create_w", "mrp_ll_ta_root_batch", "mrp_ll_ta_eps_root_batch",
           "mrp_ll_ta_eps_root_batch_stored", "mrp_ll_ta_root_batch_w", "mrp_ll_ta_eps_root_batch_w"]

_lib = None


def load_library(path: Optional[str] = None):
    """Load libmrp_ll.so (raises OSError with a build hint if it is missing — no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or _LIB_PATH
    if not os.path.exists(p):
        raise OSError(f"{p} not found: build it with `python -m libmultirobotplanning_amd._build` "
                      "(hipcc --offload-arch=gfx950); the engine has no CPU fallback")
    lib = ctypes.CDLL(p)
    lib.mrp_ll_create.restype = ctypes.c_int
    lib.mrp_ll_create.argtypes = [ctypes.POINTER(mrp_ll_options), ctypes.POINTER(ctypes.c_void_p)]
    lib.mrp_ll_destroy.restype = None
    lib.mrp_ll_destroy.argtypes = [ctypes.c_void_p]
    lib.mrp_ll_last_error.restype = ctypes.c_char_p
    lib.mrp_ll_last_error.argtypes = [ctypes.c_void_p]
    lib.mrp_ll_upload_map.restype = ctypes.c_int
    lib.mrp_ll_upload_map.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, I32P, I32P]
    lib.mrp_ll_search_batch.restype = ctypes.c_int
    lib.mrp_ll_search_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(mrp_ll_job),
                                        ctypes.POINTER(mrp_ll_result)]
    lib.mrp_ll_submit.restype = ctypes.c_int
    lib.mrp_ll_submit.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(mrp_ll_job),
                                  ctypes.POINTER(mrp_ll_result), I32P]
    lib.mrp_ll_wait.restype = ctypes.c_int
    lib.mrp_ll_wait.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mrp_ll_get_stats.restype = ctypes.c_int
    lib.mrp_ll_get_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(mrp_ll_stats)]
    lib.mrp_ll_reset_stats.restype = ctypes.c_int
    lib.mrp_ll_reset_stats.argtypes = [ctypes.c_void_p]
    lib.mrp_ll_version.restype = ctypes.c_char_p
    lib.mrp_ll_version.argtypes = []
    lib.mrp_ll_session_begin.restype = ctypes.c_int
    lib.mrp_ll_session_begin.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mrp_ll_session_begin_algo.restype = ctypes.c_int
    lib.mrp_ll_session_begin_algo.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    lib.mrp_ll_session_begin_tiers.restype = ctypes.c_int
    lib.mrp_ll_session_begin_tiers.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    lib.mrp_ll_session_tiers_geometry.restype = ctypes.c_int
    lib.mrp_ll_session_tiers_geometry.argtypes = [ctypes.c_void_p, I32P, I32P, I32P]
    lib.mrp_ll_session_front_tables.restype = ctypes.c_int
    lib.mrp_ll_session_front_tables.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mrp_ll_session_end.restype = ctypes.c_int
    lib.mrp_ll_session_end.argtypes = [ctypes.c_void_p]
    lib.mrp_ll_poll.restype = ctypes.c_int
    lib.mrp_ll_poll.argtypes = [ctypes.c_void_p, ctypes.c_int32, I32P]
    lib.mrp_ll_submit_lane.restype = ctypes.c_int
    lib.mrp_ll_submit_lane.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(mrp_ll_job),
                                       ctypes.POINTER(mrp_ll_result), I32P]
    lib.mrp_ll_sync_maps.restype = ctypes.c_int
    lib.mrp_ll_sync_maps.argtypes = [ctypes.c_void_p]
    lib.mrp_ll_release_maps.restype = ctypes.c_int
    lib.mrp_ll_release_maps.argtypes = [ctypes.c_void_p]
    lib.mrp_ll_conflict_scan.restype = ctypes.c_int
    lib.mrp_ll_conflict_scan.argtypes = [ctypes.c_void_p, ctypes.c_int32, I32P, I32P, I32P, ctypes.POINTER(mrp_ll_conflict)]
    lib.mrp_ll_path_store_reserve.restype = ctypes.c_int
    lib.mrp_ll_upload_heuristic.restype = ctypes.c_int
    lib.mrp_ll_upload_heuristic.argtypes = [ctypes.c_void_p, ctypes.c_int32, I32P, ctypes.POINTER(ctypes.c_int32)]
    lib.mrp_ll_path_store_reserve.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mrp_ll_compute_heuristics.restype = ctypes.c_int
    lib.mrp_ll_compute_heuristics.argtypes = [ctypes.c_void_p, ctypes.c_int32, I32P, I32P, I32P]
    lib.mrp_ll_read_heuristic.restype = ctypes.c_int
    lib.mrp_ll_read_heuristic.argtypes = [ctypes.c_void_p, ctypes.c_int32, I32P]
    lib.mrp_ll_heuristic_lookup.restype = ctypes.c_int
    lib.mrp_ll_heuristic_lookup.argtypes = [ctypes.c_void_p, ctypes.c_int32, I32P, I32P, I32P]
    lib.mrp_ll_sipp_table_create.restype = ctypes.c_int
    lib.mrp_ll_sipp_table_create.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    lib.mrp_ll_sipp_table_add.restype = ctypes.c_int
    lib.mrp_ll_sipp_table_add.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 4
    lib.mrp_ll_sipp_table_destroy.restype = None
    lib.mrp_ll_sipp_table_destroy.argtypes = [ctypes.c_void_p]
    lib.mrp_ll_poll_any.restype = ctypes.c_int
    lib.mrp_ll_poll_any.argtypes = [ctypes.c_void_p, I32P, ctypes.c_int32, I32P]
    lib.mrp_ll_submit_scan.restype = ctypes.c_int
    lib.mrp_ll_submit_scan.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(mrp_ll_job),
                                       ctypes.POINTER(mrp_ll_result), ctypes.POINTER(mrp_ll_conflict), I32P]
    lib.mrp_ll_constraint_store_reserve.restype = ctypes.c_int
    lib.mrp_ll_constraint_store_reserve.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    lib.mrp_ll_submit_sets.restype = ctypes.c_int
    lib.mrp_ll_submit_sets.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(mrp_ll_job),
                                       ctypes.POINTER(mrp_ll_result), ctypes.POINTER(mrp_ll_conflict),
                                       ctypes.POINTER(mrp_ll_constraint_ref), I32P]
    lib.mrp_ll_submit_node.restype = ctypes.c_int
    lib.mrp_ll_submit_node.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(mrp_ll_job),
                                       ctypes.POINTER(mrp_ll_result), ctypes.POINTER(mrp_ll_conflict),
                                       ctypes.POINTER(mrp_ll_constraint_ref), ctypes.POINTER(mrp_ll_scan_base), I32P]
    lib.mrp_ll_assign_batch.restype = ctypes.c_int
    lib.mrp_ll_assign_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(mrp_ll_assign_problem),
                                        ctypes.POINTER(mrp_ll_assign_result)]
    lib.mrp_ll_assign_series_create.restype = ctypes.c_int
    lib.mrp_ll_assign_series_create.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(mrp_ll_assign_problem),
                                                ctypes.POINTER(ctypes.c_void_p)]
    lib.mrp_ll_assign_batch_w.restype = ctypes.c_int
    lib.mrp_ll_assign_batch_w.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(mrp_ll_assign_problem_w),
                                          ctypes.POINTER(mrp_ll_assign_result)]
    lib.mrp_ll_assign_series_create_w.restype = ctypes.c_int
    lib.mrp_ll_assign_series_create_w.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(mrp_ll_assign_problem_w),
                                                  ctypes.POINTER(ctypes.c_void_p)]
    lib.mrp_ll_assign_series_next.restype = ctypes.c_int
    lib.mrp_ll_assign_series_next.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p),
                                              ctypes.POINTER(mrp_ll_assign_result)]
    lib.mrp_ll_ta_eps_root_batch.restype = ctypes.c_int
    lib.mrp_ll_ta_eps_root_batch.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_int32, ctypes.POINTER(mrp_ll_ta_root),
                                             ctypes.POINTER(mrp_ll_conflict), I32P]
    lib.mrp_ll_ta_eps_root_batch_stored.restype = ctypes.c_int
    lib.mrp_ll_ta_eps_root_batch_stored.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_int32, ctypes.POINTER(mrp_ll_ta_root),
                                                    ctypes.POINTER(mrp_ll_conflict), I32P, ctypes.POINTER(I32P)]
    lib.mrp_ll_ta_root_batch.restype = ctypes.c_int
    lib.mrp_ll_ta_root_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(mrp_ll_ta_root), I32P,
                                         ctypes.POINTER(mrp_ll_conflict)]
    lib.mrp_ll_ta_root_batch_w.restype = ctypes.c_int
    lib.mrp_ll_ta_root_batch_w.argtypes = lib.mrp_ll_ta_root_batch.argtypes
    lib.mrp_ll_ta_eps_root_batch_w.restype = ctypes.c_int
    lib.mrp_ll_ta_eps_root_batch_w.argtypes = lib.mrp_ll_ta_eps_root_batch.argtypes
    lib.mrp_ll_assign_series_destroy.restype = None
    lib.mrp_ll_assign_series_destroy.argtypes = [ctypes.c_void_p]
    if path is None:
        _lib = lib
    return lib


@dataclass
class LLJob:
    """One low-level search: LowLevelEnvironment(env, agent, constraints[, solution]) + search(start, out)."""
    map_id: int
    algo: int
    start: Sequence[int]
    goal: Optional[Sequence[int]]  # None: ASTAR_TA / ASTAR_EPS_TA for an agent without a task (MRP_LL_JOB_NO_GOAL)
    agent_idx: int = 0
    w: float = 1.0
    vertex_constraints: Sequence[Sequence[int]] = ()   # (time, x, y)
    edge_constraints: Sequence[Sequence[int]] = ()     # (time, x1, y1, x2, y2)
    ctx_paths: Sequence[Sequence[Sequence[int]]] = ()  # per agent [[x, y], ...]; [] = empty path
    max_expansions: int = -1
    collision_intervals: Sequence[Sequence[int]] = ()  # SIPP: [x, y, start, end] (grouped per location, in order)
    initial_cost: int = 0  # A*: AStar::search(..., initialCost) a_star.hpp:64; SIPP: SIPP::search(..., startTime) sipp.hpp:92
    sipp_table: Optional[int] = None  # SIPP: handle from LowLevelEngine.sipp_table_create (replaces collision_intervals)
    sipp_commit: bool = False         # SIPP with sipp_table: on success the path's stays join the table (mrp_ll.h)
    path_ids: Optional[Sequence[int]] = None  # f2: path-store slots of ctx_paths (-1 = none); lengths come from ctx_paths
    result_path_id: int = -1                  # f2: path-store slot that also receives the result path
    heuristic_id: int = -1                    # ASTAR_TA / ASTAR_EPS_TA: LowLevelEngine.upload_heuristic of the goal cell
    heavy: bool = False                       # MRP_LL_JOB_HEAVY: the search is known to outgrow the LDS tier (a hint)
    table_h: bool = False                     # MRP_LL_JOB_TABLE_H: ASTAR / ASTAR_EPS with h = table heuristic_id of the job's own goal
    try_lds: bool = False                     # MRP_LL_JOB_TRY_LDS: ASTAR_EPS_TA starts in its LDS tier (a hint; other algorithms ignore it)
    scan_conflicts: bool = False              # MRP_LL_JOB_SCAN_CONFLICTS: the node's conflicts come back too (search_batch_scan)
    # device constraint store (constraint_store_reserve): the agent's set at the parent node by its slot, and the slot that
    # receives base + vertex_constraints / edge_constraints (then the ADDITIONS); -1 = none.  Either one makes the job a
    # MRP_LL_JOB_CONSTRAINT_SET job, and the call that carries it goes through mrp_ll_submit_sets.
    base_set_id: int = -1
    result_set_id: int = -1
    # MRP_LL_JOB_SCAN_FROM_PARENT (with scan_conflicts): (parent_count, clean_before) of the parent node; path_ids[agent_idx]
    # then names the slot of the path this search replaces.  The call goes through mrp_ll_submit_node.
    scan_base: Optional[Tuple[int, int]] = None


@dataclass
class LLResult:
    status: int
    success: bool
    cost: int
    fmin: int
    expanded: int
    states: List[List[int]] = field(default_factory=list)   # [t, x, y]
    actions: List[int] = field(default_factory=list)
    tier: int = 0
    action_costs: List[int] = field(default_factory=list)
    n_states: int = 0  # mrp_ll_result.n_states as the library left it (0 unless a path came back)


@dataclass
class TaRoot:
    """One root node of a CBS-TA conflict tree (mrp_ll_ta_root): the agents' starts, and per agent its task — goal cell and
    the heuristic id of that cell's table — or None / a negative id for an agent without a task."""
    map_id: int
    starts: Sequence[Sequence[int]]
    goals: Sequence[Optional[Sequence[int]]]
    heuristic_ids: Sequence[int]
    max_expansions: int = -1


@dataclass
class TaRootResult:
    planned: int               # results filled in
    results: List[LLResult]    # per agent; NOT_RUN behind the agent the root ended at, BAD_JOB for a refused root
    conflict: dict             # as conflict_scan returns it; found = -1, the rest 0, when not every agent got a path


@dataclass
class AssignResult:
    status: int          # OK, NO_SOLUTION (infeasible; an exhausted series) or BAD_JOB
    matched: int         # pairs
    cost: int
    task_of: List[int]   # per agent, -1 = none


class AssignmentSeries:
    """One next-best series (mrp_ll_assign_series_*): every matching of the optimum's cardinality once, in non-decreasing
    order of cost; then NO_SOLUTION with matched = 0, again and again.  Made by LowLevelEngine.assign_series."""

    def __init__(self, engine, handle, n_agents):
        self._eng, self._h, self.n_agents = engine, handle, n_agents

    def next(self) -> AssignResult:
        return self._eng.assign_series_next([self])[0]

    @staticmethod
    def next_many(series: Sequence["AssignmentSeries"]) -> List[AssignResult]:
        """One step of several series of one engine: all children of all pops are solved by ONE launch."""
        return series[0]._eng.assign_series_next(series) if series else []

    def close(self):
        if self._h:
            self._eng._lib.mrp_ll_assign_series_destroy(self._h)
            self._h = None


class LowLevelEngine:
    def __init__(self, device: int = 0, n_tickets: int = 0, slots: int = 0, arena_nodes: int = 0,
                 max_horizon: int = 0, max_cells: int = 0, lds_nodes: int = 0):
        self._lib = load_library()
        opt = mrp_ll_options(device, n_tickets, slots, arena_nodes, max_horizon, max_cells, lds_nodes, 0)
        h = ctypes.c_void_p()
        rc = self._lib.mrp_ll_create(ctypes.byref(opt), ctypes.byref(h))
        if rc != 0 or not h:
            raise RuntimeError(f"mrp_ll_create failed (rc={rc}): a HIP device is required, there is no CPU fallback")
        self._h = h
        self.max_horizon = max_horizon or 512
        self._map_dims = {}  # map id -> (dimx, dimy), heuristic id -> map id: the shape read_heuristic returns
        self._heur_map = {}

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mrp_ll_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed rc={rc}: {self._lib.mrp_ll_last_error(self._h).decode()}")

    def upload_map(self, dimx, dimy, obstacles) -> int:
        ob = np.ascontiguousarray(np.asarray(obstacles, dtype=np.int32).reshape(-1, 2))
        mid = ctypes.c_int32(-1)
        self._check(self._lib.mrp_ll_upload_map(self._h, dimx, dimy, len(ob), ob.ctypes.data_as(I32P),
                                                ctypes.byref(mid)), "mrp_ll_upload_map")
        self._map_dims[mid.value] = (dimx, dimy)
        return mid.value

    def _marshal(self, jobs: Sequence[LLJob], cap: int):
        """Build the ctypes job/result arrays for `jobs`; returns (cjobs, cres, keepalive)."""
        n = len(jobs)
        cjobs = (mrp_ll_job * max(n, 1))()
        cres = (mrp_ll_result * max(n, 1))()
        keep = []
        states = np.zeros((max(n, 1), cap, 3), dtype=np.int32)
        actions = np.zeros((max(n, 1), cap), dtype=np.int32)
        costs = np.zeros((max(n, 1), cap), dtype=np.int32)
        for i, j in enumerate(jobs):
            cj = cjobs[i]
            cj.map_id, cj.algo, cj.w, cj.agent_idx = j.map_id, j.algo, j.w, j.agent_idx
            cj.start_x, cj.start_y = j.start[0], j.start[1]
            cj.goal_x, cj.goal_y = (j.goal[0], j.goal[1]) if j.goal is not None else (0, 0)
            vc = np.ascontiguousarray(np.asarray(j.vertex_constraints, dtype=np.int32).reshape(-1, 3))
            ec = np.ascontiguousarray(np.asarray(j.edge_constraints, dtype=np.int32).reshape(-1, 5))
            cj.n_vertex_constraints, cj.vertex_constraints = len(vc), vc.ctypes.data_as(I32P)
            cj.n_edge_constraints, cj.edge_constraints = len(ec), ec.ctypes.data_as(I32P)
            na = len(j.ctx_paths)
            plen = np.asarray([len(p) for p in j.ctx_paths], dtype=np.int32)
            parr = [np.ascontiguousarray(np.asarray(p, dtype=np.int32).reshape(-1, 2)) for p in j.ctx_paths]
            pptr = (I32P * max(na, 1))(*[a.ctypes.data_as(I32P) for a in parr])
            cj.n_agents = na
            cj.path_len = plen.ctypes.data_as(I32P)
            cj.path_xy = ctypes.cast(pptr, ctypes.POINTER(I32P))
            cj.max_expansions = j.max_expansions
            cj.initial_cost = j.initial_cost
            if j.sipp_table is not None:
                cj.sipp_table = j.sipp_table
                cj.sipp_commit = 1 if j.sipp_commit else 0
            cj.result_path_id = j.result_path_id
            cj.flags = (JOB_STORE_RESULT if j.result_path_id >= 0 else 0) | (JOB_NO_GOAL if j.goal is None else 0) | \
                (JOB_HEAVY if j.heavy else 0) | (JOB_SCAN_CONFLICTS if j.scan_conflicts else 0) | \
                (JOB_CONSTRAINT_SET if (j.base_set_id >= 0 or j.result_set_id >= 0) else 0) | \
                (JOB_SCAN_FROM_PARENT if j.scan_base is not None else 0) | (JOB_TRY_LDS if j.try_lds else 0) | \
                (JOB_TABLE_H if j.table_h else 0)
            cj.heuristic_id = j.heuristic_id
            if j.path_ids is not None:
                ids = np.ascontiguousarray(np.asarray(j.path_ids, dtype=np.int32))
                cj.path_ids = ids.ctypes.data_as(I32P)
                keep.append(ids)
            if j.collision_intervals:
                locs, counts, ivs = [], [], []
                for x, y, a, b in j.collision_intervals:  # consecutive entries of one location form one list
                    if locs and locs[-1] == [x, y]:
                        counts[-1] += 1
                    else:
                        locs.append([x, y])
                        counts.append(1)
                    ivs.append([a, b])
                cxy = np.ascontiguousarray(np.asarray(locs, dtype=np.int32))
                ccnt = np.ascontiguousarray(np.asarray(counts, dtype=np.int32))
                civ = np.ascontiguousarray(np.asarray(ivs, dtype=np.int32))
                cj.n_collision_locations = len(locs)
                cj.collision_xy, cj.collision_count = cxy.ctypes.data_as(I32P), ccnt.ctypes.data_as(I32P)
                cj.collision_intervals = civ.ctypes.data_as(I32P)
                keep.append((cxy, ccnt, civ))
            keep.append((vc, ec, plen, parr, pptr))
            cres[i].states_txy = states[i].ctypes.data_as(I32P)
            cres[i].actions = actions[i].ctypes.data_as(I32P)
            cres[i].states_cap = cap
            cres[i].action_costs = costs[i].ctypes.data_as(I32P)
        return cjobs, cres, (keep, states, actions, costs)

    def search_batch(self, jobs: Sequence[LLJob], states_cap: Optional[int] = None) -> List[LLResult]:
        n = len(jobs)
        cap = states_cap or self.max_horizon
        if any(j.base_set_id >= 0 or j.result_set_id >= 0 or j.scan_base is not None for j in jobs):
            return self.wait_sets(self.submit_sets(jobs, states_cap=cap), want_conflicts=False)[0]
        cjobs, cres, (keep, states, actions, costs) = self._marshal(jobs, cap)
        self._check(self._lib.mrp_ll_search_batch(self._h, n, cjobs, cres), "mrp_ll_search_batch")
        return self._results(n, cap, cres, states, actions, costs)

    def submit_sets(self, jobs: Sequence[LLJob], states_cap: Optional[int] = None, tag: int = 0):
        """mrp_ll_submit_sets, in a batch or inside any session: returns a handle for wait_sets.  Jobs with base_set_id /
        result_set_id name their constraint sets in the device store; jobs with scan_conflicts get their conflicts (the
        conflicts array is NULL when no job asks for them).  When a job carries scan_base the call is mrp_ll_submit_node."""
        n = len(jobs)
        cap = states_cap or self.max_horizon
        cjobs, cres, bufs = self._marshal(jobs, cap)
        conf = None
        if any(j.scan_conflicts for j in jobs):
            conf = (mrp_ll_conflict * max(n, 1))()
            for c in conf:
                for k, _ in mrp_ll_conflict._fields_:
                    setattr(c, k, SCAN_UNTOUCHED)
        sets = (mrp_ll_constraint_ref * max(n, 1))()
        for i, j in enumerate(jobs):
            sets[i].base_set_id, sets[i].result_set_id = j.base_set_id, j.result_set_id
        ticket = ctypes.c_int32(-1)
        if any(j.scan_base is not None for j in jobs):
            bases = (mrp_ll_scan_base * max(n, 1))()
            for i, j in enumerate(jobs):
                if j.scan_base is not None:
                    bases[i].parent_count, bases[i].clean_before = j.scan_base
            self._check(self._lib.mrp_ll_submit_node(self._h, tag, n, cjobs, cres, conf, sets, bases, ctypes.byref(ticket)),
                        "mrp_ll_submit_node")
            return (ticket.value, n, cap, cjobs, cres, conf, (sets, bases), bufs)
        self._check(self._lib.mrp_ll_submit_sets(self._h, tag, n, cjobs, cres, conf, sets, ctypes.byref(ticket)),
                    "mrp_ll_submit_sets")
        return (ticket.value, n, cap, cjobs, cres, conf, sets, bufs)

    def wait_sets(self, handle, want_conflicts: bool = True):
        """mrp_ll_wait for a submit_sets handle: (results, conflicts) as search_batch_scan returns them (conflicts is None
        when they are not wanted; every entry is SCAN_UNTOUCHED when no job of the call asked for a scan)."""
        ticket, n, cap, cjobs, cres, conf, sets, (keep, states, actions, costs) = handle
        self._check(self._lib.mrp_ll_wait(self._h, ticket), "mrp_ll_wait")
        res = self._results(n, cap, cres, states, actions, costs)
        if not want_conflicts:
            return res, None
        names = [k for k, _ in mrp_ll_conflict._fields_]
        return res, [{k: (getattr(conf[i], k) if conf is not None else SCAN_UNTOUCHED) for k in names} for i in range(n)]

    def search_batch_scan(self, jobs: Sequence[LLJob], states_cap: Optional[int] = None, tag: int = 0):
        """mrp_ll_submit_scan + mrp_ll_wait, in a batch or inside any session: returns (results, conflicts).  conflicts[i] is
        a dict as conflict_scan returns for a job with scan_conflicts (found = -1, the rest 0, when the job did not end
        with a path); every field of a job without the flag keeps SCAN_UNTOUCHED, the value the array was filled with."""
        n = len(jobs)
        cap = states_cap or self.max_horizon
        if any(j.base_set_id >= 0 or j.result_set_id >= 0 or j.scan_base is not None for j in jobs):
            return self.wait_sets(self.submit_sets(jobs, states_cap=cap, tag=tag))
        cjobs, cres, (keep, states, actions, costs) = self._marshal(jobs, cap)
        conf = (mrp_ll_conflict * max(n, 1))()
        for c in conf:
            for k, _ in mrp_ll_conflict._fields_:
                setattr(c, k, SCAN_UNTOUCHED)
        ticket = ctypes.c_int32(-1)
        self._check(self._lib.mrp_ll_submit_scan(self._h, tag, n, cjobs, cres, conf, ctypes.byref(ticket)), "mrp_ll_submit_scan")
        self._check(self._lib.mrp_ll_wait(self._h, ticket.value), "mrp_ll_wait")
        return (self._results(n, cap, cres, states, actions, costs),
                [{k: getattr(conf[i], k) for k, _ in mrp_ll_conflict._fields_} for i in range(n)])

    @staticmethod
    def _results(n, cap, cres, states, actions, costs) -> List[LLResult]:
        out = []
        for i in range(n):
            r = cres[i]
            ns = r.n_states if r.status in (OK, PATH_TRUNCATED) else 0
            m = min(ns, cap)
            out.append(LLResult(status=r.status, success=r.status in (OK, PATH_TRUNCATED), cost=r.cost, fmin=r.fmin,
                                expanded=r.expanded, states=states[i, :m].tolist(),
                                actions=actions[i, :max(m - 1, 0)].tolist(), tier=r.tier,
                                action_costs=costs[i, :max(m - 1, 0)].tolist(), n_states=r.n_states))
        return out

    def conflict_scan(self, solutions: Sequence[Sequence[Sequence[Sequence[int]]]]) -> List[dict]:
        """getFirstConflict (example/ecbs.cpp:401-452) + focalHeuristic (:315-350) for a batch of solutions, each a list
        of paths [[x, y], ...].  Returns per solution dict(found, time, agent1, agent2, type, x1, y1, x2, y2, count)."""
        n = len(solutions)
        set_first = np.zeros(n + 1, dtype=np.int32)
        lens = []
        for s, sol in enumerate(solutions):
            set_first[s + 1] = set_first[s] + len(sol)
            lens.extend(len(p) for p in sol)
        path_first = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(np.asarray(lens, dtype=np.int64), out=path_first[1:])
        flat = [xy for sol in solutions for p in sol for xy in p]
        xy = np.ascontiguousarray(np.asarray(flat, dtype=np.int32).reshape(-1, 2))
        out = (mrp_ll_conflict * max(n, 1))()
        self._check(self._lib.mrp_ll_conflict_scan(self._h, n, set_first.ctypes.data_as(I32P),
                                                   path_first.ctypes.data_as(I32P), xy.ctypes.data_as(I32P), out),
                    "mrp_ll_conflict_scan")
        return [{k: getattr(out[i], k) for k, _ in mrp_ll_conflict._fields_} for i in range(n)]

    def _marshal_ta_roots(self, roots: Sequence[TaRoot], cap: int):
        """The ctypes arrays of mrp_ll_ta_root_batch for `roots`: (croots, planned, conflicts, per-root result buffers, keepalive)."""
        n = len(roots)
        croots = (mrp_ll_ta_root * max(n, 1))()
        planned = np.full(max(n, 1), -7, dtype=np.int32)
        conf = (mrp_ll_conflict * max(n, 1))()
        keep, per_root = [], []
        for i, r in enumerate(roots):
            na = len(r.starts)
            st = np.ascontiguousarray(np.asarray(r.starts, dtype=np.int32).reshape(-1, 2))
            hid = np.ascontiguousarray(np.asarray(r.heuristic_ids, dtype=np.int32).reshape(-1))
            gl = np.ascontiguousarray(np.asarray([g if g is not None else (0, 0) for g in r.goals], dtype=np.int32).reshape(-1, 2))
            cres = (mrp_ll_result * max(na, 1))()
            states = np.zeros((max(na, 1), cap, 3), dtype=np.int32)
            actions = np.zeros((max(na, 1), cap), dtype=np.int32)
            costs = np.zeros((max(na, 1), cap), dtype=np.int32)
            for a in range(na):
                cres[a].states_txy = states[a].ctypes.data_as(I32P)
                cres[a].actions = actions[a].ctypes.data_as(I32P)
                cres[a].states_cap = cap
                cres[a].action_costs = costs[a].ctypes.data_as(I32P)
            c = croots[i]
            c.map_id, c.n_agents, c.max_expansions = r.map_id, na, r.max_expansions
            c.starts_xy, c.goals_xy, c.heuristic_ids = st.ctypes.data_as(I32P), gl.ctypes.data_as(I32P), hid.ctypes.data_as(I32P)
            c.results = ctypes.cast(cres, ctypes.POINTER(mrp_ll_result))
            keep.append((st, hid, gl))
            per_root.append((na, cres, states, actions, costs))
        return croots, planned, conf, per_root, keep

    def ta_root_batch(self, roots: Sequence[TaRoot], states_cap: Optional[int] = None, raw_rc: bool = False, wide: bool = False):
        """mrp_ll_ta_root_batch: the roots of CBS-TA conflict trees, one workgroup each, in one launch.  Returns one
        TaRootResult per root; with raw_rc the call's return code instead of raising (E_BUSY inside a session).
        wide: mrp_ll_ta_root_batch_w (roots of up to 256 agents instead of 64; the same answers)."""
        n = len(roots)
        cap = states_cap or self.max_horizon
        croots, planned, conf, per_root, keep = self._marshal_ta_roots(roots, cap)
        call = self._lib.mrp_ll_ta_root_batch_w if wide else self._lib.mrp_ll_ta_root_batch
        rc = call(self._h, n, croots, planned.ctypes.data_as(I32P), conf)
        if raw_rc and rc != 0:
            return rc
        self._check(rc, "mrp_ll_ta_root_batch_w" if wide else "mrp_ll_ta_root_batch")
        names = [k for k, _ in mrp_ll_conflict._fields_]
        return [TaRootResult(planned=int(planned[i]), results=self._results(na, cap, cres, states, actions, costs),
                             conflict={k: getattr(conf[i], k) for k in names})
                for i, (na, cres, states, actions, costs) in enumerate(per_root)]

    def ta_eps_root_batch(self, roots: Sequence[TaRoot], w: float, states_cap: Optional[int] = None, raw_rc: bool = False,
                          result_path_ids: Optional[Sequence[Optional[Sequence[int]]]] = None, wide: bool = False):
        """mrp_ll_ta_eps_root_batch: the roots of ECBS-TA conflict trees under weight w, one workgroup each, in one launch:
        agent a's MRP_LL_ASTAR_EPS_TA search sees the paths of the agents before it.  Returns one TaRootResult per root
        (conflict["count"] is the node's focalHeuristic); with raw_rc the call's return code instead of raising.
        result_path_ids (mrp_ll_ta_eps_root_batch_stored): per root None or one path-store slot per agent (-1: not stored)
        that also receives the agent's path, for later jobs that name it in path_ids; the answer is the same.
        wide: mrp_ll_ta_eps_root_batch_w (roots of up to 256 agents instead of 64; the same answers); it has no stored
        variant, so wide together with result_path_ids raises ValueError."""
        if wide and result_path_ids is not None:
            raise ValueError("ta_eps_root_batch: the wide call stores no paths (wide=True with result_path_ids)")
        n = len(roots)
        cap = states_cap or self.max_horizon
        croots, planned, conf, per_root, keep = self._marshal_ta_roots(roots, cap)
        if result_path_ids is not None:
            if len(result_path_ids) != n:
                raise ValueError("result_path_ids: one entry per root")
            arrs = [None if ids is None else np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1)) for ids in result_path_ids]
            for r, a in zip(roots, arrs):
                if a is not None and len(a) != len(r.starts):
                    raise ValueError("result_path_ids: one slot per agent")
            ptrs = (I32P * max(n, 1))(*[a.ctypes.data_as(I32P) if a is not None else I32P() for a in arrs])
            keep.append((arrs, ptrs))
            rc = self._lib.mrp_ll_ta_eps_root_batch_stored(self._h, w, n, croots, conf, planned.ctypes.data_as(I32P), ptrs)
        elif wide:
            rc = self._lib.mrp_ll_ta_eps_root_batch_w(self._h, w, n, croots, conf, planned.ctypes.data_as(I32P))
        else:
            rc = self._lib.mrp_ll_ta_eps_root_batch(self._h, w, n, croots, conf, planned.ctypes.data_as(I32P))
        if raw_rc and rc != 0:
            return rc
        self._check(rc, "mrp_ll_ta_eps_root_batch")
        names = [k for k, _ in mrp_ll_conflict._fields_]
        return [TaRootResult(planned=int(planned[i]), results=self._results(na, cap, cres, states, actions, costs),
                             conflict={k: getattr(conf[i], k) for k in names})
                for i, (na, cres, states, actions, costs) in enumerate(per_root)]

    def upload_heuristic(self, map_id: int, dist) -> int:
        """MRP_LL_ASTAR_TA: the shortest-path table of one goal cell, dist[dimy][dimx] (INT32_MAX = unreachable)."""
        d = np.ascontiguousarray(np.asarray(dist, dtype=np.int64).clip(-1, 2 ** 31 - 1).astype(np.int32).reshape(-1))
        hid = ctypes.c_int32(-1)
        self._check(self._lib.mrp_ll_upload_heuristic(self._h, map_id, d.ctypes.data_as(I32P), ctypes.byref(hid)),
                    "mrp_ll_upload_heuristic")
        self._heur_map[hid.value] = map_id
        return hid.value

    def compute_heuristics(self, map_ids: Sequence[int], goals: Sequence[Sequence[int]]) -> List[int]:
        """mrp_ll_compute_heuristics: the shortest-path tables of goals[k] = (x, y) on map map_ids[k], computed on the
        device from the uploaded maps in one launch; returns their heuristic ids (as upload_heuristic's)."""
        mids = np.ascontiguousarray(np.asarray(map_ids, dtype=np.int32).reshape(-1))
        gxy = np.ascontiguousarray(np.asarray(goals, dtype=np.int32).reshape(-1, 2))
        if len(mids) != len(gxy):
            raise ValueError("compute_heuristics: one goal per map id")
        hids = np.full(max(len(mids), 1), -1, dtype=np.int32)
        self._check(self._lib.mrp_ll_compute_heuristics(self._h, len(mids), mids.ctypes.data_as(I32P),
                                                        gxy.ctypes.data_as(I32P), hids.ctypes.data_as(I32P)),
                    "mrp_ll_compute_heuristics")
        out = hids[:len(mids)].tolist()
        self._heur_map.update(zip(out, mids.tolist()))
        return out

    def read_heuristic(self, hid: int) -> np.ndarray:
        """mrp_ll_read_heuristic: table `hid` (computed or uploaded) as an int32 array [dimy, dimx], INT32_MAX =
        unreachable."""
        mid = self._heur_map.get(hid)
        if mid is None:
            raise ValueError("read_heuristic: unknown heuristic id %r" % (hid,))
        dimx, dimy = self._map_dims[mid]
        dist = np.zeros((dimy, dimx), dtype=np.int32)
        self._check(self._lib.mrp_ll_read_heuristic(self._h, hid, dist.ctypes.data_as(I32P)), "mrp_ll_read_heuristic")
        return dist

    def heuristic_lookup(self, hids: Sequence[int], cells: Sequence[Sequence[int]]) -> np.ndarray:
        """mrp_ll_heuristic_lookup: out[k] = table hids[k] at cells[k] = (x, y) (INT32_MAX = unreachable) — the entries of
        the assignment's cost matrix without moving whole tables."""
        ids = np.ascontiguousarray(np.asarray(hids, dtype=np.int32).reshape(-1))
        cxy = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 2))
        if len(ids) != len(cxy):
            raise ValueError("heuristic_lookup: one cell per heuristic id")
        out = np.zeros(max(len(ids), 1), dtype=np.int32)
        self._check(self._lib.mrp_ll_heuristic_lookup(self._h, len(ids), ids.ctypes.data_as(I32P), cxy.ctypes.data_as(I32P),
                                                      out.ctypes.data_as(I32P)), "mrp_ll_heuristic_lookup")
        return out[:len(ids)]

    def _marshal_assign(self, problems, wide=False):
        """dicts -> mrp_ll_assign_problem[].  Matrix form: cost ([nA][nT]; None or ASSIGN_NO_EDGE = no edge); gather form:
        heuristic_ids [nT], starts [nA][2], allowed [nA] (optional).  Both: forbidden [nA], mode [nA], min_matching.
        wide: -> mrp_ll_assign_problem_w[]; a mask is a Python int of any width, marshalled to mask_words =
        ceil(n_tasks / 64) words (at least one; its bits at or above 64 * mask_words are dropped)."""
        n = len(problems)
        carr = ((mrp_ll_assign_problem_w if wide else mrp_ll_assign_problem) * max(n, 1))()
        keep, dims = [], []

        def arr(v, dtype, ptr, shape=-1):
            a = np.ascontiguousarray(np.asarray(v, dtype=dtype).reshape(shape))
            if a.size == 0:
                a = np.zeros(1, dtype=dtype)
            keep.append(a)
            return a.ctypes.data_as(ptr)

        def masks(v, words):
            if not wide:
                return arr(v, np.uint64, U64P)
            return arr([[(int(m) >> (64 * k)) & (2 ** 64 - 1) for k in range(words)] for m in v], np.uint64, U64P)

        for c, p in zip(carr, problems):
            cost = p.get("cost")
            if cost is not None:
                if not isinstance(cost, np.ndarray):
                    cost = np.array([[ASSIGN_NO_EDGE if v is None else v for v in row] for row in cost], dtype=np.int64)
                    cost = cost.reshape((int(p["nA"]), int(p["nT"])) if "nA" in p else (len(cost), -1 if len(cost) else 0))
                if cost.ndim != 2:
                    raise ValueError("assign: cost must be [n_agents][n_tasks]")
                c.n_agents, c.n_tasks = (int(p["nA"]), int(p["nT"])) if "nA" in p else cost.shape
                if cost.size and (cost.min() < -2 ** 31 or cost.max() >= 2 ** 31):
                    raise ValueError("assign: a cost does not fit 32 bits")
                c.cost = arr(cost, np.int32, I32P)
            else:
                c.n_agents, c.n_tasks = len(p["starts"]), len(p["heuristic_ids"])
                c.heuristic_ids = arr(p["heuristic_ids"], np.int32, I32P)
                c.starts_xy = arr(p["starts"], np.int32, I32P)
            words = min(max((c.n_tasks + 63) // 64, 1), 4)
            if wide:
                c.mask_words = int(p.get("mask_words", words))  # (tests hand in a wrong one)
            if cost is None and p.get("allowed") is not None:
                c.allowed = masks(p["allowed"], words)
            if p.get("forbidden") is not None:
                c.forbidden = masks(p["forbidden"], words)
            if p.get("mode") is not None:
                c.mode = arr(p["mode"], np.int32, I32P)
            c.min_matching = int(p.get("min_matching") or 0)
            dims.append(c.n_agents)
        return carr, keep, dims

    @staticmethod
    def _assign_results(dims):
        cres = (mrp_ll_assign_result * max(len(dims), 1))()
        task_of = [np.full(max(min(d, 4096), 1), -1, dtype=np.int32) for d in dims]
        for r, t in zip(cres, task_of):
            r.task_of = t.ctypes.data_as(I32P)
        return cres, task_of

    @staticmethod
    def _assign_unpack(cres, task_of, dims):
        return [AssignResult(r.status, r.matched, r.cost, t[:max(min(d, len(t)), 0)].tolist()) for r, t, d in zip(cres, task_of, dims)]

    def assign_batch(self, problems: Sequence[dict], wide: bool = False) -> List[AssignResult]:
        """mrp_ll_assign_batch: every problem's maximum-cardinality, minimum-cost matching, the whole batch in ONE launch.
        A rejected problem comes back with status BAD_JOB; the others are unaffected.  wide: mrp_ll_assign_batch_w, up to
        256 agents x 256 tasks per problem (narrow: 64 x 64), masks as Python ints of any width."""
        carr, keep, dims = self._marshal_assign(problems, wide)
        cres, task_of = self._assign_results(dims)
        if wide:
            self._check(self._lib.mrp_ll_assign_batch_w(self._h, len(problems), carr, cres), "mrp_ll_assign_batch_w")
        else:
            self._check(self._lib.mrp_ll_assign_batch(self._h, len(problems), carr, cres), "mrp_ll_assign_batch")
        return self._assign_unpack(cres, task_of, dims)

    def assign_series(self, problems: Sequence[dict], wide: bool = False) -> List[AssignmentSeries]:
        """mrp_ll_assign_series_create: one next-best series per (unconstrained) problem; the optima in ONE launch.
        wide: mrp_ll_assign_series_create_w (up to 256 x 256)."""
        carr, keep, dims = self._marshal_assign(problems, wide)
        hs = (ctypes.c_void_p * max(len(problems), 1))()
        if wide:
            self._check(self._lib.mrp_ll_assign_series_create_w(self._h, len(problems), carr, hs), "mrp_ll_assign_series_create_w")
        else:
            self._check(self._lib.mrp_ll_assign_series_create(self._h, len(problems), carr, hs), "mrp_ll_assign_series_create")
        return [AssignmentSeries(self, hs[k], dims[k]) for k in range(len(problems))]

    def assign_series_next(self, series: Sequence[AssignmentSeries]) -> List[AssignResult]:
        """mrp_ll_assign_series_next: the next matching of each series; all children of all pops in ONE launch — narrow and
        wide series may be mixed, then the narrow children take one launch and the wide children another."""
        dims = [s.n_agents for s in series]
        hs = (ctypes.c_void_p * max(len(series), 1))(*[s._h for s in series])
        cres, task_of = self._assign_results(dims)
        self._check(self._lib.mrp_ll_assign_series_next(self._h, len(series), hs, cres), "mrp_ll_assign_series_next")
        return self._assign_unpack(cres, task_of, dims)

    def sync_maps(self) -> None:
        """mrp_ll_sync_maps: copy what has been uploaded so far to the device now (otherwise done by the next submit)."""
        self._check(self._lib.mrp_ll_sync_maps(self._h), "mrp_ll_sync_maps")

    def release_maps(self) -> None:
        """mrp_ll_release_maps: forget every map and heuristic table; ids start again at 0."""
        self._check(self._lib.mrp_ll_release_maps(self._h), "mrp_ll_release_maps")
        self._map_dims.clear()
        self._heur_map.clear()

    def path_store_reserve(self, n_slots: int) -> None:
        """Allocate the device-resident path store (f2): slots 0..n_slots-1 are the caller's to hand out."""
        self._check(self._lib.mrp_ll_path_store_reserve(self._h, n_slots), "mrp_ll_path_store_reserve")

    def constraint_store_reserve(self, n_slots: int, words_per_slot: int) -> None:
        """Allocate the device-resident constraint store: n_slots sets of up to words_per_slot (<= 2048) packed words."""
        self._check(self._lib.mrp_ll_constraint_store_reserve(self._h, n_slots, words_per_slot),
                    "mrp_ll_constraint_store_reserve")

    def sipp_table_create(self, map_id: int) -> int:
        h = ctypes.c_void_p()
        self._check(self._lib.mrp_ll_sipp_table_create(self._h, map_id, ctypes.byref(h)), "mrp_ll_sipp_table_create")
        return h.value

    def sipp_table_add(self, table: int, x: int, y: int, start: int, end: int) -> None:
        self._check(self._lib.mrp_ll_sipp_table_add(table, x, y, start, end), "mrp_ll_sipp_table_add")

    def sipp_table_destroy(self, table: int) -> None:
        self._lib.mrp_ll_sipp_table_destroy(table)

    def session_occupancy(self, algo: int) -> int:
        """mrp_ll_session_occupancy: resident searches per CU of a session of `algo`."""
        occ = ctypes.c_int32(0)
        self._check(self._lib.mrp_ll_session_occupancy(self._h, algo, ctypes.byref(occ)), "mrp_ll_session_occupancy")
        return occ.value

    def session_front_tables(self, in_memory: bool) -> None:
        """mrp_ll_session_front_tables: the front workgroups of a front / heavy session keep focal tables in device memory."""
        self._check(self._lib.mrp_ll_session_front_tables(self._h, 1 if in_memory else 0), "mrp_ll_session_front_tables")

    def session_tiers_geometry(self):
        """mrp_ll_session_tiers_geometry: (front workgroups per CU, front window bytes, heavy window bytes)."""
        occ, front, heavy = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.mrp_ll_session_tiers_geometry(self._h, ctypes.byref(occ), ctypes.byref(front), ctypes.byref(heavy)),
                    "mrp_ll_session_tiers_geometry")
        return occ.value, front.value, heavy.value

    def configure_tiers(self, lds_nodes: int = 0, lds_rows: int = 0, lds_path_bytes: int = 0) -> int:
        """Geometry of the LDS fast tier for the launches that follow (0 = keep); returns resident searches per CU."""
        occ = ctypes.c_int32(0)
        self._check(self._lib.mrp_ll_configure_tiers(self._h, lds_nodes, lds_rows, lds_path_bytes, ctypes.byref(occ)),
                    "mrp_ll_configure_tiers")
        return occ.value

    def session_begin(self, workgroups: int = 0):
        """Keep `workgroups` wavefronts resident and feed them through the host job ring (see mrp_ll.h)."""
        self._check(self._lib.mrp_ll_session_begin(self._h, workgroups), "mrp_ll_session_begin")

    def session_begin_algo(self, algo: int, workgroups: int = 0):
        """A session for jobs of one algorithm only (the specialised resident kernel)."""
        self._check(self._lib.mrp_ll_session_begin_algo(self._h, algo, workgroups), "mrp_ll_session_begin_algo")

    def session_begin_tiers(self, workgroups: int, heavy_workgroups: int):
        """An A*-epsilon session as a pair of resident launches: front workgroups (LDS tier only) + heavy workgroups (wide
        LDS tier, arena tier) that take over the searches that outgrow the front tier (include/mrp_ll.h)."""
        self._check(self._lib.mrp_ll_session_begin_tiers(self._h, ASTAR_EPS, workgroups, heavy_workgroups),
                    "mrp_ll_session_begin_tiers")

    def session_begin_sipp(self, workgroups: int = 0):
        """A session for MRP_LL_SIPP jobs (resident SIPP kernel); other jobs come back as BAD_JOB."""
        self._check(self._lib.mrp_ll_session_begin_sipp(self._h, workgroups), "mrp_ll_session_begin_sipp")

    def session_end(self):
        self._check(self._lib.mrp_ll_session_end(self._h), "mrp_ll_session_end")

    def stats(self) -> dict:
        st = mrp_ll_stats()
        self._check(self._lib.mrp_ll_get_stats(self._h, ctypes.byref(st)), "mrp_ll_get_stats")
        return {k: (list(getattr(st, k)) if k == "prof" else getattr(st, k)) for k, _ in mrp_ll_stats._fields_}

    def reset_stats(self):
        self._check(self._lib.mrp_ll_reset_stats(self._h), "mrp_ll_reset_stats")
