/*
 * mrp_ll.h — C ABI of the MI355X low-level search engine (libmrp_ll.so).
 *
 * Drop-in boundary for ONE path of Sartor02/libMultiRobotPlanning: the per-agent low-level search that the
 * conflict-tree searches call once per agent and once per conflict-tree child.  The reference has no FFI at this
 * point — the boundary is a compile-time template concept — so each entry point below names the reference
 * interface it replaces:
 *
 *   LowLevelSearch_t::search(const State& start, PlanResult& out)
 *       CBS  : AStar<State,Action,Cost,LowLevelEnvironment>            cbs.hpp:248, called at cbs.hpp:99-101,155-157
 *       ECBS : AStarEpsilon<State,Action,Cost,LowLevelEnvironment>(w)  ecbs.hpp:421-422, called at ecbs.hpp:126-129,265-268
 *       search bodies: a_star.hpp:63-161, a_star_epsilon.hpp:86-285
 *   LowLevelEnvironment(env, agentIdx, constraints[, solution])        cbs.hpp:209-217, ecbs.hpp:365-375
 *       -> Environment::setLowLevelContext                              example/ecbs.cpp:264-274, example/cbs.cpp:266-276
 *   Environment::{admissibleHeuristic,isSolution,getNeighbors,stateValid,transitionValid,
 *                 focalStateHeuristic,focalTransitionHeuristic}         example/ecbs.cpp:276-312,352-399,497-510
 *   PlanResult{states,actions,cost,fmin}                                planresult.hpp:18-27
 *   Environment::onExpandLowLevelNode (the metric's numerator)          example/ecbs.cpp:476-479
 *
 * Because a device cannot call back into C++ templates, everything the search reads is passed explicitly in
 * mrp_ll_job: the static map, the agent's start/goal, its vertex/edge constraint sets and (ECBS) the other agents'
 * current paths that the focal heuristics consult.  Jobs of one batch are independent; results are bit-identical to
 * the reference's integers (cost, fmin, path, expansion count) for the grid MAPF Environment of example/ecbs.cpp and
 * example/cbs.cpp.  All buffers are caller-owned; no pointer outlives the call that received it (for
 * mrp_ll_submit: the matching mrp_ll_wait).
 *
 * A context is NOT thread-safe; use one per host thread.  There is no CPU fallback: every entry point fails with
 * MRP_LL_E_DEVICE when no HIP device is usable.
 */
#ifndef MRP_LL_H
#define MRP_LL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes of the API calls ------------------------------------------------------------------------- */
#define MRP_LL_SUCCESS 0
#define MRP_LL_E_INVALID (-1)  /* bad argument (NULL pointer, unknown map id, dimension out of range, ...)   */
#define MRP_LL_E_DEVICE (-2)   /* HIP error / no device; see mrp_ll_last_error()                            */
#define MRP_LL_E_NOMEM (-3)
#define MRP_LL_E_BUSY (-4)     /* no free ticket for mrp_ll_submit                                          */

/* ---- search algorithm of a job ----------------------------------------------------------------------------- */
#define MRP_LL_ASTAR 0     /* a_star.hpp AStar::search          (CBS low level)  */
#define MRP_LL_ASTAR_EPS 1 /* a_star_epsilon.hpp AStarEpsilon   (ECBS low level) */
#define MRP_LL_SIPP 2      /* sipp.hpp SIPP::search over the grid Environment of example/mapf_prioritized_sipp.cpp;  */
                           /* a batch (or a session, mrp_ll_session_begin_sipp) holds either SIPP jobs or A-star     */
                           /* jobs, not both.                                                                        */
                           /* Inside the limits below a job comes back with the reference's integers (status, cost,    */
                           /* fmin, expansions, states, actions, action costs); beyond one it comes back with the named */
                           /* status and without a path.  Limits:                                                       */
                           /*   times       every arrival time the search GENERATES is at most 1023 (the 10-bit g field): */
                           /*               a successor that would arrive later ends the job with MRP_LL_CAP_HORIZON     */
                           /*               whatever max_horizon is, even when the reference's answer does not use that   */
                           /*               successor (a neighbour's safe interval that starts at 1024 is enough).        */
                           /*               initial_cost (the start time) is at most 1023, else MRP_LL_BAD_JOB.           */
                           /*   path        the raw A* solution — one state per move, before the explicit Waits of       */
                           /*               sipp.hpp:105-128 are inserted — has at most max_horizon / 2 states           */
                           /*               -> MRP_LL_CAP_HORIZON.  (With the Waits it has up to max_horizon - 1 states:  */
                           /*               a smaller states_cap gives MRP_LL_PATH_TRUNCATED.)                            */
                           /*   nodes       at most arena_nodes (cell, safe interval) states are created, the start      */
                           /*               included -> MRP_LL_CAP_NODES.                                                 */
                           /*   table       a table that travels with its job (the collision_* arrays, a sipp_table outside */
                           /*               a session or one that does not fit the resident layout) with K listed cells    */
                           /*               and S safe intervals on them in all must satisfy                              */
                           /*                 4 * ((dimx * dimy + 1) / 2 + K + 1 + 2 * S) <= 131072  (bytes of the slot's  */
                           /*                 table area) and  dimx * dimy + S <= max_horizon * ((max_cells + 31) / 32)   */
                           /*               -> MRP_LL_CAP_NODES before the search starts (on 255 x 255: K + 2 * S <= 254). */
                           /*   resident    a sipp_table stays on the device (mrp_ll_session_begin_sipp) while every cell  */
                           /*               has at most 15 safe intervals and every finite bound of a safe interval is     */
                           /*               below 65535; otherwise it travels whole, under the table limit above.  Same   */
                           /*               results either way.                                                          */
                           /* result.tier (diagnostic): 1 = run in the arena (every job whose table travels, and a job that  */
                           /* ended before its search began: no safe interval at the start time); on a resident table 0 =  */
                           /* finished in the LDS tier (up to 767 nodes), 2 = finished in the middle tier (node records in  */
                           /* the arena, up to 1152 open entries in LDS), 3 = finished in the arena after both.  A search   */
                           /* moves on when the next expansion might not fit: 60 free node records and open entries (four   */
                           /* neighbours x 15 intervals) are wanted before every expansion.                                  */

#define MRP_LL_ASTAR_TA 3  /* a_star.hpp AStar::search over the Environment of example/cbs_ta.cpp:283-372 — the low level of */
                           /* CBS with task assignment ONLY (cbs_ta.hpp:106-109,155-158,196-199; ecbs_ta.hpp runs          */
                           /* AStarEpsilon over the same Environment: MRP_LL_ASTAR_EPS_TA below): optional goal            */
                           /* (MRP_LL_JOB_NO_GOAL), h = a shortest-path table (mrp_ll_upload_heuristic, or computed on the   */
                           /* device: mrp_ll_compute_heuristics), Wait costs 0 at the goal, so g != time and decrease-key is live. */
                           /* Two tiers, like the other searches: the LDS tier (maps up to 32 x 32, at most 64 vertex and  */
                           /* 64 edge constraints, time steps <= 61, f <= 254, 1023 open nodes) and, for everything beyond */
                           /* it, the arena tier.  "Time steps <= 61" is about the nodes the tier EXPANDS: a node that ends   */
                           /* the search is popped, not expanded, so a solution whose last state has time 62 (63 states)     */
                           /* still finishes in the LDS tier, one with time 63 does not.  Likewise f and h <= 254 are asked   */
                           /* of every node the tier generates and of the start, and "1023 open nodes" means: before an       */
                           /* expansion the open list, the popped node included, has room for five more.  The expansion cap   */
                           /* is tested first at every pop: a search that ends MRP_LL_CAP_EXPANSIONS there is the tier's own   */
                           /* answer.  The arena tier takes any map the context accepts, any number of constraints; limits:  */
                           /* mrp_ll_options.arena_nodes / max_horizon — MRP_LL_CAP_NODES / MRP_LL_CAP_HORIZON — and as many */
                           /* time steps as arena_nodes x 4 status words hold: 512 on a 32 x 32 map by default).            */

#define MRP_LL_ASTAR_EPS_TA 4 /* a_star_epsilon.hpp AStarEpsilon::search over the Environment of example/ecbs_ta.cpp:283-445 */
                           /* — the low level of ECBS with task assignment (ecbs_ta.hpp:498-499; calls :126-128, :278, :321). */
                           /* Goal, heuristic_id and MRP_LL_JOB_NO_GOAL as for MRP_LL_ASTAR_TA; w, agent_idx, n_agents,        */
                           /* path_len and path_xy (the shipped focal context) as for MRP_LL_ASTAR_EPS.  The focal heuristics   */
                           /* look the other agents up at the successor's TIME (g != time here).  A state found again with a  */
                           /* smaller g is re-keyed in the open list and, if it already sits in the focal list, keeps its      */
                           /* place there with the new key (a_star_epsilon.hpp:249-269), exactly as the reference's heaps do.   */
                           /* The device-resident path store serves it as it serves MRP_LL_ASTAR_EPS: with                     */
                           /* MRP_LL_JOB_STORE_RESULT the result path also stays in slot result_path_id, and path_ids names    */
                           /* the context's paths by their slots instead of shipping them (path_xy may be NULL) — under the    */
                           /* same rules: a store is reserved, the id of every other agent with path_len > 0 lies inside it,  */
                           /* the longest path_len is at most max_horizon, and the table [longest path_len][n_agents rounded   */
                           /* up to 16] of 2-byte cells fits the arena slot's path area (the workgroup builds it there).       */
                           /* Rejected (MRP_LL_BAD_JOB): initial_cost != 0, MRP_LL_JOB_ROOT_CHAIN, _HEAVY, _SCAN_CONFLICTS,    */
                           /* _CONSTRAINT_SET; path_ids or _STORE_RESULT with no store reserved.                              */
                           /* Runs in batches and in mixed sessions (mrp_ll_session_begin); the one-algorithm                  */
                           /* sessions and mrp_ll_session_occupancy answer MRP_LL_E_INVALID for it.                          */
                           /* Two tiers.  With MRP_LL_JOB_TRY_LDS the search starts in the LDS tier (result.tier == 0): maps   */
                           /* up to 32 x 32, at most 64 vertex and 64 edge constraints (after the packer dropped those        */
                           /* outside the map or the horizon), at most 128 context agents (n_agents rounded up to 16), and a  */
                           /* launch with the LDS tier on and lds_path_bytes >= 4096 (mrp_ll_configure_tiers; the default).   */
                           /* Inside it: 1023 nodes, 1023 open and 1023 focal entries (room for five more of each is asked    */
                           /* in front of every expansion), expanded nodes at t <= min(61, lds_rows - 2), f and h <= 124,     */
                           /* focalH <= 511.  A job that does not fit is not tried there; a search that outgrows the tier is  */
                           /* run again from the start by the arena tier (result.tier == 1) — no limit of the LDS tier is     */
                           /* ever an answer.  Without the flag:                                                              */
                           /* one tier, the arena (result.tier == 1): any map the context accepts, any number of              */
                           /* constraints, any number of context agents.  Limits, with B = 40 * arena_nodes + 48 bytes:       */
                           /*   time steps  min(max_horizon, B / (8 * dimx * dimy))            -> MRP_LL_CAP_HORIZON          */
                           /*   nodes       (B - 4 * time steps * dimx * dimy - 64) / 48       -> MRP_LL_CAP_NODES            */
                           /*   g <= 1023, f <= 2045 (MRP_LL_CAP_HORIZON), focalH <= 2047 (MRP_LL_CAP_FOCAL)                  */
                           /* By default (arena_nodes 131072, max_horizon 512): 512 time steps and 65 534 nodes on a          */
                           /* 32 x 32 map, 284 and 54 698 on 48 x 48, 160 and 54 613 on 64 x 64.                              */

/* ---- per-job status (mrp_ll_result.status) ----------------------------------------------------------------- */
#define MRP_LL_OK 0             /* search() returned true                                                    */
#define MRP_LL_NO_SOLUTION 1    /* search() returned false: open list exhausted (a_star.hpp:160)              */
#define MRP_LL_CAP_EXPANSIONS 2 /* job.max_expansions exceeded (the reference has no cap and would keep going) */
#define MRP_LL_CAP_NODES 3      /* per-search node arena exhausted (mrp_ll_options.arena_nodes)               */
#define MRP_LL_CAP_HORIZON 4    /* a state beyond mrp_ll_options.max_horizon would have been generated         */
#define MRP_LL_BAD_JOB 5        /* job rejected on the host (unknown map, start/goal outside the grid, ...)    */
#define MRP_LL_PATH_TRUNCATED 6 /* solved, but result.states_cap was too small; cost/fmin/expanded are valid    */
#define MRP_LL_NOT_RUN 8        /* root chain (MRP_LL_JOB_ROOT_CHAIN): the chain ended before this agent's search            */
#define MRP_LL_CAP_FOCAL 7      /* a node's focal value exceeded the 11-bit key field (2047 accumulated conflicts)  */

/* Action codes == enum class Action of example/ecbs.cpp:49-55 */
#define MRP_LL_ACT_UP 0
#define MRP_LL_ACT_DOWN 1
#define MRP_LL_ACT_LEFT 2
#define MRP_LL_ACT_RIGHT 3
#define MRP_LL_ACT_WAIT 4

typedef struct mrp_ll_ctx mrp_ll_ctx;

typedef struct mrp_ll_options {
  int32_t device;          /* HIP device ordinal                                                             */
  int32_t n_tickets;       /* batches that may be in flight at once (0 = default 4)                           */
  int32_t slots;           /* resident searches per in-flight batch (0 = default 1024)                        */
  int32_t arena_nodes;     /* HBM node capacity per search before MRP_LL_CAP_NODES (0 = default 131072)       */
  int32_t max_horizon;     /* largest state time + 1 (0 = default 512, max 1024)                              */
  int32_t max_cells;       /* largest dimx*dimy accepted by mrp_ll_upload_map (0 = default 4096, max 65025)   */
  int32_t lds_nodes;       /* 2 x open-list entries of the LDS-resident fast tier (0 = default 2048, <0 = no tier) */
  int32_t reserved;
} mrp_ll_options;

/* One low-level search == one LowLevelEnvironment + one LowLevelSearch_t::search call of the reference. */
typedef struct mrp_ll_job {
  int32_t map_id;  /* from mrp_ll_upload_map                                                                  */
  int32_t algo;    /* MRP_LL_ASTAR | MRP_LL_ASTAR_EPS                                                         */
  float w;         /* suboptimality bound, binary32 exactly as AStarEpsilon::m_w (a_star_epsilon.hpp:386)      */
  int32_t agent_idx; /* index of this agent inside `path_*` (its own entry is ignored, ecbs.cpp:287)          */
  int32_t start_x, start_y; /* start State is (time 0, x, y)  (ecbs.cpp:571)                                  */
  int32_t goal_x, goal_y;   /* m_goals[agentIdx]              (ecbs.cpp:573)                                  */
  int32_t n_vertex_constraints;
  const int32_t* vertex_constraints; /* [n][3] = time, x, y           (ecbs.cpp:108-112)                      */
  int32_t n_edge_constraints;
  const int32_t* edge_constraints;   /* [n][5] = time, x1, y1, x2, y2 (ecbs.cpp:140-147)                      */
  /* ECBS focal context: the CT node's `solution` vector (ecbs.hpp:381-389). Ignored for MRP_LL_ASTAR. */
  int32_t n_agents;                  /* solution.size(); 0 = no context                                       */
  const int32_t* path_len;           /* [n_agents] states per path; 0 = empty path, skipped (ecbs.cpp:287)    */
  const int32_t* const* path_xy;     /* [n_agents] -> [path_len][2] = x, y at time 0,1,2,...                  */
  int64_t max_expansions;            /* < 0: unlimited                                                        */
  /* MRP_LL_SIPP only — SIPP::setCollisionIntervals (sipp.hpp:82-85,245-284), one entry per location; a location
   * given twice keeps the later list.  Ignored by the other algorithms (leave zero). */
  int32_t n_collision_locations;
  const int32_t* collision_xy;        /* [n][2]   x, y                                                        */
  const int32_t* collision_count;     /* [n]      intervals of that location                                  */
  const int32_t* collision_intervals; /* [sum][2] start, end (inclusive; end may be INT32_MAX)                 */
  /* The fork's extra search arguments (both default to 0 in the reference):
   *   MRP_LL_ASTAR     : AStar::search(start, solution, initialCost)   a_star.hpp:63-64,78,100 — the start node's gScore;
   *                      cost and fmin come back offset by it (a start that already is the goal keeps fmin = h(start),
   *                      because the start node's fScore is pushed without it, a_star.hpp:78)
   *   MRP_LL_SIPP      : SIPP::search(start, waitAction, solution, startTime)  sipp.hpp:92-103 — the safe interval of the
   *                      start cell is looked up at this time, state times are absolute, cost = arrival - startTime
   *   MRP_LL_ASTAR_EPS : AStarEpsilon::search has no such argument: a non-zero value is rejected (MRP_LL_BAD_JOB) */
  int32_t initial_cost;
  /* MRP_LL_SIPP with sipp_table: 1 = when the search succeeds, the stays of the path it found become collision
   * intervals of the table — [t_k, t_{k+1} - 1] on the k-th cell of the path, [t_last, INT32_MAX] on the last — exactly
   * the mrp_ll_sipp_table_add calls a prioritized planner makes with the solution (mapf_prioritized_sipp.cpp:237-246),
   * done by the engine (in a session: by the workgroup that ran the search, on the device-resident table).  The table
   * then has ONE user at a time: the next job on it is submitted after this one's result has been collected. */
  int32_t sipp_commit;
  /* MRP_LL_SIPP only, optional: an incrementally maintained table (mrp_ll_sipp_table_*) instead of the collision_*
   * arrays above (which are then ignored).  The table must stay unchanged until the job has been submitted. */
  const struct mrp_ll_sipp_table* sipp_table;
  /* Device-resident path store (mrp_ll_path_store_reserve).  A conflict-tree child differs from its
   * parent in ONE path (ecbs.hpp:253-263 copies all N), and every path was produced by a search of this engine: with
   * result_path_id >= 0 the kernel ALSO leaves the result path in that store slot, and a later MRP_LL_ASTAR_EPS or
   * MRP_LL_ASTAR_EPS_TA job names the CT node's paths by their slots — path_ids[n_agents], -1 = no path / the searching
   * agent itself — instead of shipping them (path_xy may then be NULL; path_len is still required).  Slot ids are managed
   * by the caller: a slot may be reused once no unfinished job names it.
   * A slot is a length word and max_horizon states (rounded up to 8 halfwords), and the packer cannot know a result's
   * length beforehand: the device stores NOTHING when a path does not fit its slot, and the slot keeps its previous
   * content, which a by-id reader would then take for the path.  A caller that stores results keeps its paths below
   * max_horizon and treats a returned n_states >= max_horizon as "not stored".
   * result_path_id is honoured only when `flags` has MRP_LL_JOB_STORE_RESULT: a zero-initialised job (`mrp_ll_job j{}`,
   * memset) stores nothing and touches no slot. */
  const int32_t* path_ids;
  int32_t result_path_id;  /* with MRP_LL_JOB_STORE_RESULT: the slot (0 .. n_slots-1) that also receives the result path */
  int32_t flags;           /* MRP_LL_JOB_* bits; 0 = none */
  /* MRP_LL_ASTAR_TA / _EPS_TA: the shortest-path table of this job's goal cell (mrp_ll_upload_heuristic or mrp_ll_compute_heuristics); ignored with
   * MRP_LL_JOB_NO_GOAL.  MRP_LL_ASTAR / _EPS: the same with MRP_LL_JOB_TABLE_H.  (Zero-initialised jobs of the other algorithms never look at it.) */
  int32_t heuristic_id;
  int32_t chain_count;     /* MRP_LL_JOB_ROOT_CHAIN: plan at most this many agents (0 = all from agent_idx on): a caller with many
                            * agents cuts the root step into jobs of bounded length; the agents behind come back MRP_LL_NOT_RUN */
  /* MRP_LL_JOB_ROOT_CHAIN only: [n_agents][4] = start x, start y, goal x, goal y of every agent of the instance. */
  const int32_t* chain_starts_goals_xy;
} mrp_ll_job;

#define MRP_LL_JOB_STORE_RESULT 1 /* mrp_ll_job.flags: also leave the result path in path-store slot result_path_id */
/* MRP_LL_JOB_ROOT_CHAIN (sessions of MRP_LL_ASTAR_EPS with a path store; maps up to 32 x 32, at most 128 agents, and room
 * for the 64-row focal table of all agents in the LDS window — mrp_ll_configure_tiers' lds_path_bytes): ONE job
 * that is the root step of an ECBS conflict tree (ecbs.hpp:118-136) from agent `agent_idx` on: agent a = agent_idx ..
 * n_agents - 1 is planned with no constraints against the paths of the agents 0 .. a - 1, one after the other, by one
 * workgroup that keeps the focal context in LDS.  path_ids[n_agents] names the path-store slot of EVERY agent: where the
 * paths of the agents before agent_idx are, and where the others' paths go (all >= 0).  max_expansions is the budget of
 * the whole chain (each search gets what the ones before it left, like a caller that subtracts `expanded` itself).
 * The job's result has chain_results -> [n_agents - agent_idx] ordinary results (each with its own buffers), filled in
 * agent order: the chain ends BEHIND an agent whose search found no path or exceeded the budget, and IN FRONT OF one
 * whose search outgrows the LDS tier — that one and every later agent come back as MRP_LL_NOT_RUN and are the caller's to
 * submit as ordinary jobs (or as another chain).  The job's own n_states = results filled in, expanded = their sum.
 * Every filled-in result is exactly what the ordinary job for that agent would have returned.
 * When agent_idx == 0 and every agent got a path, the workgroup — which holds the whole root solution in LDS — also scans
 * it for conflicts (Environment::getFirstConflict ecbs.cpp:401-452, focalHeuristic ecbs.cpp:315-350): the job's own
 * cost = number of conflicts (0: the root node is the solution, the conflict tree has nothing to do) and fmin = the first
 * one as  time << 24 | type << 16 | agent1 << 8 | agent2  (type 0 vertex / 1 edge), or -1 if there is none; both are -1
 * when the scan did not take place (a chain that is cut by chain_count or starts behind agent 0 does not scan).
 * A budget that has nothing left does not end the chain by itself: the next search starts with max_expansions = 0, like an
 * ordinary job, and comes back MRP_LL_CAP_EXPANSIONS with expanded = 1 (the expansion that exceeded it).
 * A chain that is refused — outside such a session (a batch, a mixed session), on a larger map, with a slot id outside the
 * store, ... — runs nothing and touches no slot: status MRP_LL_BAD_JOB, n_states = 0, expanded = 0, cost = fmin = -1, and
 * every entry of chain_results MRP_LL_NOT_RUN with its other fields 0. */
#define MRP_LL_JOB_ROOT_CHAIN 4
/* MRP_LL_JOB_HEAVY (hint, MRP_LL_ASTAR_EPS): the caller knows that this search outgrows the LDS tier every search starts in
 * (e.g. a root chain ended in front of it): no attempt is made there.  Results never depend on it. */
#define MRP_LL_JOB_HEAVY 8
/* MRP_LL_JOB_SCAN_CONFLICTS (mrp_ll_submit_scan below; MRP_LL_ASTAR_EPS jobs whose context names every other agent's path by its
 * path-store slot): the workgroup that finishes the search also scans the conflict-tree node the job completes — the new
 * path in place of agent_idx's, path_ids' paths for everybody else — and returns its first conflict and its number of
 * conflicts with the result.  Combines with MRP_LL_JOB_HEAVY and MRP_LL_JOB_STORE_RESULT; never changes a result. */
#define MRP_LL_JOB_SCAN_CONFLICTS 16
/* MRP_LL_JOB_TRY_LDS (hint, MRP_LL_ASTAR_EPS_TA; the other algorithms ignore it): start the search in that algorithm's LDS
 * tier (see MRP_LL_ASTAR_EPS_TA above).  No result field but `tier` (0: finished in the LDS tier, 1: arena) ever depends on
 * it.  Combines with MRP_LL_JOB_NO_GOAL, MRP_LL_JOB_STORE_RESULT and path_ids. */
#define MRP_LL_JOB_TRY_LDS 128
/* MRP_LL_JOB_TABLE_H (MRP_LL_ASTAR and MRP_LL_ASTAR_EPS; the other algorithms ignore it, as they ignore MRP_LL_JOB_TRY_LDS):
 * admissibleHeuristic(s) is the value of the shortest-path table heuristic_id (mrp_ll_upload_heuristic or
 * mrp_ll_compute_heuristics) at s's cell instead of the Manhattan distance of ecbs.cpp:276-279 — what example/cbs.cpp:445-557
 * carries switched off.  Everything else of the search is example/ecbs.cpp / example/cbs.cpp as without the flag: neighbour
 * order, unit costs (g == time), isSolution by the goal and m_lastGoalConstraint, the focal heuristics, the heaps' tie order,
 * the binary32 bound, fmin, the expansion count; initial_cost works for MRP_LL_ASTAR as it does without the flag.  (A flag,
 * because a zero-initialised job has heuristic_id == 0, which is a valid id.)
 * The engine does not know which cell a table was made for: naming the table of the job's OWN goal is the caller's duty.  A
 * table of another cell (of the same map) may give a wrong path and nothing else: no access outside the job's buffers, no
 * search that ignores its caps.
 * A start whose table value is "unreachable" cannot reach the goal at all (a reachable cell has only reachable neighbours, so
 * the case arises nowhere else): the job comes back MRP_LL_NO_SOLUTION with expanded == 0 and no path, where the Manhattan
 * search would run into a cap.
 * Limit: f = g + h of the start and of every generated successor is at most 2045 (the arena tier's heap entry has an 11-bit f
 * field; the Manhattan h is bounded by the map and never had to be tested).  A start or a successor beyond it ends the job
 * MRP_LL_CAP_HORIZON, as it does for the task-assignment searches.  The other limits are those of the job without the flag:
 * arena_nodes -> MRP_LL_CAP_NODES, max_horizon -> MRP_LL_CAP_HORIZON.  Any map the context accepts.
 * Two tiers, as without the flag.  On a map up to 32 x 32, with at most 64 edge constraints and 128 context agents, under a
 * launch with the LDS tier on and lds_path_bytes >= 2048 (mrp_ll_configure_tiers; the default is 4096), the search starts in
 * the narrow LDS tier (result.tier == 0): the table's 2048 bytes stand in the window's path area, together with the focal path
 * table where both fit (otherwise the focal table is read from the arena slot).  Inside it: 1023 open entries, expanded nodes at
 * t <= 61, focalH <= 511, and f <= 124 for the start and for every generated successor (the tier's 7-bit f field).  A search
 * that outgrows one of these is run again from the start by the arena tier (result.tier == 1) — no limit of the LDS tier is ever
 * an answer.  A job that is answered before any search (the unreachable start above) reports tier 1.  The wide LDS geometry of
 * the heavy workgroups and the one-algorithm kernels have no table form.
 * MRP_LL_BAD_JOB, never a silent Manhattan search: heuristic_id unknown or of another map than map_id; the flag together
 * with MRP_LL_JOB_STORE_RESULT, _ROOT_CHAIN, _HEAVY, _SCAN_CONFLICTS, _SCAN_FROM_PARENT or _CONSTRAINT_SET, or with
 * path_ids; a flagged job in a one-algorithm session (mrp_ll_session_begin_algo / _tiers / _tiers_gated).  Runs in
 * mrp_ll_search_batch / mrp_ll_submit and in mixed sessions (mrp_ll_session_begin); a batch that holds a flagged job runs in
 * the mixed kernel. */
#define MRP_LL_JOB_TABLE_H 256
#define MRP_LL_JOB_NO_GOAL 2      /* mrp_ll_job.flags, MRP_LL_ASTAR_TA: the agent has no task (cbs_ta.cpp:283-319: h = 0, every
                                   * cell ends the search once time > the agent's last vertex constraint, every Wait is free) */

typedef struct mrp_ll_result {
  int32_t status;   /* MRP_LL_OK ... */
  int32_t cost;     /* PlanResult::cost  (valid when status == MRP_LL_OK / MRP_LL_PATH_TRUNCATED)             */
  int32_t fmin;     /* PlanResult::fmin  (a_star_epsilon.hpp:210, a_star.hpp:104)                              */
  int32_t n_states; /* PlanResult::states.size(); actions.size() == n_states - 1                              */
  int64_t expanded; /* calls of onExpandNode during this search (counts the goal pop)                         */
  int32_t* states_txy; /* caller buffer [states_cap][3] = time, x, y ; may be NULL                            */
  int32_t* actions;    /* caller buffer [states_cap]    = MRP_LL_ACT_* ; may be NULL                          */
  int32_t states_cap;
  int32_t tier;     /* 0 = finished in the LDS tier, 1 = run by the arena tier, 2 = by a heavy workgroup's wide LDS tier (diagnostic; MRP_LL_SIPP: 0 / 2 / 3 / 1, see MRP_LL_SIPP above) */
  int32_t* action_costs; /* caller buffer [states_cap] or NULL: PlanResult::actions[k].second (always 1 for
                          * MRP_LL_ASTAR / _EPS; 0 for a Wait at the goal with MRP_LL_ASTAR_TA; Wait durations for
                          * MRP_LL_SIPP, sipp.hpp:105-128)                                                     */
  struct mrp_ll_result* chain_results; /* MRP_LL_JOB_ROOT_CHAIN jobs only: caller array [n_agents - agent_idx]  */
} mrp_ll_result;

typedef struct mrp_ll_stats {
  int64_t launches;          /* kernel launches so far                                                        */
  int64_t jobs;              /* searches run                                                                  */
  int64_t expansions;        /* low-level expansions summed over all searches                                 */
  int64_t nodes_created;     /* heap pushes summed over all searches                                          */
  int64_t migrated;          /* searches that left the LDS tier                                               */
  double kernel_ms;          /* sum of hipEvent-measured kernel durations (on the launching stream)           */
  double h2d_ms, d2h_ms;     /* hipEvent-measured copy durations                                              */
  double session_busy_ms, session_idle_ms; /* session mode: sum over resident workgroups of time in jobs / waiting */
  int64_t session_active_wgs;              /* session mode: workgroups that ran at least one job (summed over sessions) */
  double pack_ms, unpack_ms; /* host time spent packing jobs (mrp_ll_submit) / unpacking results (mrp_ll_wait)           */
  int64_t staged_bytes;      /* bytes of job descriptors, constraint words, id lists and path / interval tables written   */
                             /* to pinned host memory for the device to read over PCIe                                    */
  int64_t prof[8];           /* diagnostic (-DMRP_LL_TRACE library only, else 0): shader cycles in walk, pops,  */
                             /* pushes, successor generation, row init, whole job; #walks; nodes visited by walks */
  double heavy_busy_ms, heavy_idle_ms;     /* mrp_ll_session_begin_tiers: the same two sums over the heavy workgroups    */
  int64_t heavy_active_wgs;                /* ... and how many of them ran at least one search                           */
  int64_t heavy_fallbacks;                 /* sessions that fell back to a single launch (no heavy workgroup became resident) */
} mrp_ll_stats;

int mrp_ll_create(const mrp_ll_options* opt, mrp_ll_ctx** out);
void mrp_ll_destroy(mrp_ll_ctx* ctx);
const char* mrp_ll_last_error(const mrp_ll_ctx* ctx);

/* Static map (Environment ctor, ecbs.cpp:249-259): obstacles as [n][2] = x, y.  Uploaded once, used by any job. */
int mrp_ll_upload_map(mrp_ll_ctx* ctx, int32_t dimx, int32_t dimy, int32_t n_obstacles, const int32_t* obstacles_xy,
                      int32_t* map_id);

/* MRP_LL_ASTAR_TA: the heuristic of one goal cell of map `map_id` — dist[dimy][dimx] (row-major, dist[y * dimx + x]) =
 * ShortestPathHeuristic::getValue(cell, goal) (example/shortest_path_heuristic.hpp:56-60: all-pairs shortest paths on the
 * free cells; INT32_MAX = unreachable), computed by the caller (the reference does it once per Environment,
 * cbs_ta.cpp:267); the engine keeps it next to the maps (any map size).  A caller without a table of its own lets the
 * device compute it from the uploaded map: mrp_ll_compute_heuristics below.  MRP_LL_E_BUSY during a session. */
int mrp_ll_upload_heuristic(mrp_ll_ctx* ctx, int32_t map_id, const int32_t* dist, int32_t* heuristic_id);

/* The same tables computed where they are consumed: n tables in ONE kernel launch (one wavefront each, whatever n is),
 * table k = ShortestPathHeuristic::getValue(cell, goal k) (example/shortest_path_heuristic.hpp:12-63) on map map_ids[k]
 * for the goal cell goals_xy[k] = x, y.  The graph is the reference's (shortest_path_heuristic.hpp:22-45: a vertex per cell,
 * an edge between two horizontally or vertically adjacent cells when BOTH are free), and Floyd-Warshall's d[v][v] = 0 holds
 * for every vertex: a goal on an obstacle cell gives 0 at that cell and unreachable everywhere else.  heuristic_ids[k] are
 * ordinary heuristic ids — interchangeable with mrp_ll_upload_heuristic's in mrp_ll_job.heuristic_id — and stay valid, like
 * those, until mrp_ll_release_maps; the tables live on the device only (no host copy is made or kept) and survive every
 * later upload or computation, also when the device buffer has to grow.
 * MRP_LL_E_INVALID: NULL pointer, unknown map id, goal outside its map — no id is created, the context is unchanged.
 * MRP_LL_E_BUSY while a session is active or a batch is in flight (the buffer may have to grow).  n == 0 succeeds. */
int mrp_ll_compute_heuristics(mrp_ll_ctx* ctx, int32_t n, const int32_t* map_ids, const int32_t* goals_xy /* [n][2] */,
                              int32_t* heuristic_ids /* [n] */);
/* One table back on the host: dist[dimy][dimx] as mrp_ll_upload_heuristic takes it (dist[y * dimx + x], INT32_MAX =
 * unreachable), for computed AND uploaded ids (an uploaded value beyond 65534 comes back as INT32_MAX: the table holds
 * halfwords).  MRP_LL_E_INVALID: NULL pointer, unknown id.  MRP_LL_E_BUSY as above. */
int mrp_ll_read_heuristic(mrp_ll_ctx* ctx, int32_t heuristic_id, int32_t* dist);
/* out[k] = table heuristic_ids[k] at the cell cells_xy[k] = x, y (INT32_MAX = unreachable): what the assignment's cost
 * matrix needs — cost(agent i, task j) = getValue(start_i, goal_j), example/cbs_ta.cpp:272-279 — in one gather launch and
 * one copy of n words, without moving a table.  MRP_LL_E_INVALID: NULL pointer, unknown id, cell outside the table's map.
 * MRP_LL_E_BUSY as above.  n == 0 succeeds. */
int mrp_ll_heuristic_lookup(mrp_ll_ctx* ctx, int32_t n, const int32_t* heuristic_ids, const int32_t* cells_xy /* [n][2] */,
                            int32_t* out /* [n] */);

/* ---- min-cost task assignment and its next-best series -------------------------------------------------------
 * What sits between that cost matrix and the task-assignment searches: Assignment::solve (assignment.hpp:81-118) and
 * the ordered series NextBestAssignment::solve / nextSolution (next_best_assignment.hpp:49-122) that
 * Environment::nextTaskAssignment (example/cbs_ta.cpp:442-456) asks for every new root of the conflict tree.  The
 * reference solves a min-cost flow with Boost.Graph; here ONE wavefront solves one problem (shortest augmenting paths
 * with potentials, integers only, exact) and a batch of problems is ONE kernel launch.
 *
 * A problem: n_agents x n_tasks, 0 .. 64 each.  An edge agent -> task exists where the cost is not
 * MRP_LL_ASSIGN_NO_EDGE; a cost is 0 .. 16 777 215 (2^24 - 1).  The result is a matching of MAXIMUM CARDINALITY and,
 * among those, of MINIMUM TOTAL COST; an agent may stay without a task (task_of = -1).  (Not "agents row by row": with
 * a0->t0: 2 and a1->t0: 1 the answer is {a1: t0}, cost 1.)
 * The cost rows come from `cost`, or — cost == NULL, the gather form — straight from heuristic tables that live on the
 * device: cost(a, t) = table heuristic_ids[t] at the cell starts_xy[a], for the tasks t whose bit is set in allowed[a]
 * (the goals agent a may take, cbs_ta.cpp:272-279; NULL = all).  All tables of one problem belong to one map.
 * DIFFERENCE from the reference: an unreachable goal (the table says "no path") is NO EDGE — such a pair cannot be
 * chosen; the reference hands INT_MAX to the flow solver as a cost and then fails in the search.
 * Constraints (a node of the next-best series; NULL / 0 = none): forbidden[a] is a mask of tasks agent a must not get;
 * mode[a] is MRP_LL_ASSIGN_FREE, a task the agent is forced to (>= 0), MRP_LL_ASSIGN_NO_TASK (must stay without) or
 * MRP_LL_ASSIGN_SOME_TASK (must get one); min_matching is the cardinality the matching must reach.
 * status: MRP_LL_OK; MRP_LL_NO_SOLUTION — infeasible: a forced pair has no edge or is forbidden, two agents are forced to
 * one task, a must-get agent cannot get one, or fewer than min_matching pairs (matched = 0, cost = 0, task_of all -1);
 * MRP_LL_BAD_JOB — the problem was rejected on the host and not run, the rest of the batch is unaffected: a dimension
 * outside 0 .. 64, a cost outside 0 .. 2^24 - 1, a forced task >= n_tasks or an unknown mode, min_matching outside
 * 0 .. 64, a NULL array the form needs, an unknown heuristic id, a start outside its table's map, tables of different
 * maps.  A problem's result depends on the problem alone, never on its place in the batch.
 * n_agents == 0 or n_tasks == 0 is solved with 0 pairs and cost 0. */
#define MRP_LL_ASSIGN_NO_EDGE INT32_MAX
#define MRP_LL_ASSIGN_FREE (-1)        /* mode[a]; >= 0: forced to that task */
#define MRP_LL_ASSIGN_NO_TASK (-2)     /* must stay without a task */
#define MRP_LL_ASSIGN_SOME_TASK (-3)   /* must get a task */
typedef struct mrp_ll_assign_problem {
  int32_t n_agents, n_tasks;
  const int32_t* cost;            /* [n_agents][n_tasks], or NULL: the gather form below */
  const int32_t* heuristic_ids;   /* [n_tasks]      gather form */
  const int32_t* starts_xy;       /* [n_agents][2]  gather form */
  const uint64_t* allowed;        /* [n_agents] or NULL = all;  gather form */
  const uint64_t* forbidden;      /* [n_agents] or NULL */
  const int32_t* mode;            /* [n_agents] or NULL = all free */
  int32_t min_matching;           /* 0 = none */
} mrp_ll_assign_problem;
typedef struct mrp_ll_assign_result {
  int32_t status;                 /* MRP_LL_OK | MRP_LL_NO_SOLUTION (infeasible) | MRP_LL_BAD_JOB */
  int32_t matched;                /* pairs */
  int64_t cost;
  int32_t* task_of;               /* caller buffer [n_agents]; -1 = none */
} mrp_ll_assign_result;
/* n problems in ONE launch, whatever n is (n == 0 succeeds without one).  MRP_LL_E_INVALID: a NULL argument (also a
 * NULL task_of of a problem with agents).  MRP_LL_E_BUSY while a session is active or a batch is in flight, as
 * mrp_ll_heuristic_lookup. */
int mrp_ll_assign_batch(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results);

/* The next-best series: every matching of the optimum's cardinality K, each exactly once, in non-decreasing order of
 * total cost.  Many series advance together, because a batched conflict-tree driver asks for "the next assignment" of
 * whichever instances just exhausted a root.
 * mrp_ll_assign_series_create copies n problems (mode, forbidden and min_matching must be unset: MRP_LL_E_INVALID
 * otherwise, and for a problem mrp_ll_assign_batch would reject) and solves the n optima in one launch.  A gather-form
 * series keeps reading the device's tables for every later step: its cost matrix never visits the host, and its
 * heuristic ids must stay valid while it lives.
 * mrp_ll_assign_series_next pops the cheapest open node of each of the n series (distinct: MRP_LL_E_INVALID otherwise),
 * hands its matching back and solves all children of all n pops in ONE launch (next_best_assignment.hpp:79-119: for
 * every agent i not fixed by the node, in index order, the agents before i keep what the popped matching gave them and
 * agent i must differ; a child that is infeasible or has fewer than K pairs is dropped).  An exhausted series returns
 * MRP_LL_NO_SOLUTION with matched = 0 and keeps doing so; a series whose K is 0 returns the empty matching once.
 * ORDER AMONG EQUAL COSTS: the series pops the node that was created first.  This rule — and the lowest-lane rule of
 * the wave program for equally near tasks — replaces the accidental order of Boost's path search in the reference;
 * with it the whole series is a function of the problem alone.
 * Both calls: MRP_LL_E_BUSY as mrp_ll_assign_batch.  A series belongs to the context that created it and must be
 * destroyed before that context. */
typedef struct mrp_ll_assign_series mrp_ll_assign_series;
int mrp_ll_assign_series_create(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem* problems,
                                mrp_ll_assign_series** out /* [n] */);
int mrp_ll_assign_series_next(mrp_ll_ctx* ctx, int32_t n, mrp_ll_assign_series* const* series,
                              mrp_ll_assign_result* results /* [n] */);
void mrp_ll_assign_series_destroy(mrp_ll_assign_series* series);

/* ---- the wide form: up to 256 agents x 256 tasks ---------------------------------------------------------------
 * The calls above give one lane to each agent and each task, hence 64 x 64.  The _w calls solve the same problem with
 * the same method, contract, statuses and tie rules for dimensions 0 .. 256: lane l owns the columns and agents
 * l + 64k.  They are separate calls; nothing above changes.  On a problem that fits 64 x 64 a _w call returns exactly
 * what the narrow call returns, task_of entry for entry (among equally near tasks the lowest task INDEX wins).
 * mrp_ll_assign_problem_w is mrp_ll_assign_problem plus mask_words: allowed and forbidden are [n_agents][mask_words]
 * words, bit t of an agent's mask is bit t % 64 of its word t / 64.  mask_words is 1 .. 4 and, when a mask is given, at
 * least ceil(n_tasks / 64).  Mask bits at or above n_tasks are ignored.  min_matching is 0 .. 256, a forced task
 * < n_tasks, a cost 0 .. 2^24 - 1; beyond those limits the problem is MRP_LL_BAD_JOB (MRP_LL_E_INVALID from
 * mrp_ll_assign_series_create_w).  Everything else is as the narrow calls: ONE launch per call, none for n == 0, a
 * result that depends on the problem alone, MRP_LL_E_BUSY under the same rules.
 * Where the cost rows live is a pure function of (n_agents, n_tasks, budget): in LDS when n_agents rows of
 * 256 * ceil(max(n_agents, n_tasks) / 64) bytes fit the budget (128 x 128 at the default 64 KiB), otherwise in device
 * memory (256 x 256) — the staged matrix, or for the gather form a matrix the wave writes first.  The answer is the
 * same either way.  MRP_LL_ASSIGN_LDS_BYTES (0 .. 65536, read once by mrp_ll_create) lowers the budget: a tuning and
 * test knob, 0 sends every problem with agents to memory rows.
 * A series made by mrp_ll_assign_series_create_w is advanced and destroyed by the calls above, also together with
 * narrow series in one mrp_ll_assign_series_next: the children of the narrow series go in one launch and those of the
 * wide series in another (one launch when all series are of one kind). */
typedef struct mrp_ll_assign_problem_w {
  int32_t n_agents, n_tasks;      /* 0 .. 256 */
  const int32_t* cost;
  const int32_t* heuristic_ids;
  const int32_t* starts_xy;
  const uint64_t* allowed;        /* [n_agents][mask_words] or NULL = all;  gather form */
  const uint64_t* forbidden;      /* [n_agents][mask_words] or NULL */
  const int32_t* mode;
  int32_t min_matching;
  int32_t mask_words;             /* 1 .. 4 */
} mrp_ll_assign_problem_w;
int mrp_ll_assign_batch_w(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_result* results);
int mrp_ll_assign_series_create_w(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem_w* problems,
                                  mrp_ll_assign_series** out /* [n] */);

/* Copies every map uploaded so far to the device now (otherwise done lazily by the next submit / session_begin). */
int mrp_ll_sync_maps(mrp_ll_ctx* ctx);

/* Allocates the device-resident path store: n_slots slots of one path each (up to mrp_ll_options.max_horizon states).
 * Slot ids 0 .. n_slots-1 are the caller's to hand out (mrp_ll_job.result_path_id / path_ids).  MRP_LL_E_BUSY while a
 * batch or a session is in flight; calling it again re-allocates (contents are lost). */
int mrp_ll_path_store_reserve(mrp_ll_ctx* ctx, int32_t n_slots);

/* ---- incrementally maintained SIPP tables --------------------------------------------------------------------
 * The state SIPP::setCollisionIntervals (sipp.hpp:245-284) builds up, kept by the engine so that a planner which adds a
 * few collision intervals between two searches (example/mapf_prioritized_sipp.cpp:237-246) does not have to hand over —
 * and the engine re-derive — every interval of every location for every job.  mrp_ll_sipp_table_add(t, x, y, s, e)
 * appends [s, e] to that location's collision list and is equivalent to calling setCollisionIntervals(location, list)
 * with the extended list.  A table belongs to one map (its dimensions); it is not thread-safe.
 * In a session (mrp_ll_session_begin_sipp) the table also has a DEVICE-RESIDENT copy: a job on it carries only the cells
 * changed since the table's previous job, and the search reads the copy in place (up to 15 safe intervals per cell, bounds below 65535; a
 * table that needs more, and any table outside a session, travels whole with each job — same results).  One job per
 * table is in flight at a time (a second one simply travels whole).  mrp_ll_job.sipp_commit lets the engine add the
 * found path's stays itself. */
typedef struct mrp_ll_sipp_table mrp_ll_sipp_table;
int mrp_ll_sipp_table_create(mrp_ll_ctx* ctx, int32_t map_id, mrp_ll_sipp_table** out);
int mrp_ll_sipp_table_add(mrp_ll_sipp_table* t, int32_t x, int32_t y, int32_t start, int32_t end);
void mrp_ll_sipp_table_destroy(mrp_ll_sipp_table* t);

/* Forgets every uploaded map (host copy and device buffer contents; map ids start again at 0).  For callers that keep
 * one context across many batches of instances.  MRP_LL_E_BUSY while a batch or a session is in flight. */
int mrp_ll_release_maps(mrp_ll_ctx* ctx);

/* Limits of the LDS-resident fast tier for the launches / sessions that follow.  The tier keeps a whole search in LDS
 * (open list, focal list, walk queue, a (time, cell) bitmap of 64 time steps) in a window of fixed size, plus
 * lds_path_bytes for the focal path table of a search (a larger table is read from the search's arena slot); it serves
 * maps up to 32 x 32 and focal contexts of up to 128 agents.  lds_nodes / 2 = open-list entries a search may hold inside
 * the tier (at most 1023; lds_nodes is kept as a multiple of 4, rounded DOWN, and at least 8, so the number of entries is
 * even below 1023: asking for 2 * 485 gives 484), lds_rows = time steps it may use (8 .. 64: a search leaves the tier when it is about to expand a
 * node that is no goal at a time beyond lds_rows - 2, and beyond 61 in any case); a search that outgrows a limit is run by the
 * arena tier instead (a root chain ends in front of it).  0 = keep the current value; lds_nodes < 0 disables the tier.
 * Results never depend on any of this.  *occupancy_out (may be NULL) receives the resident searches per CU (160 KiB / window + table).  MRP_LL_E_BUSY
 * while a batch or a session is in flight. */
int mrp_ll_configure_tiers(mrp_ll_ctx* ctx, int32_t lds_nodes, int32_t lds_rows, int32_t lds_path_bytes,
                           int32_t* occupancy_out);

/* Resident searches per CU of a session of `algo` (MRP_LL_ASTAR_EPS, MRP_LL_ASTAR, MRP_LL_ASTAR_TA or MRP_LL_SIPP) with the
 * current tier limits, as the HIP runtime grants them: what a caller sizes mrp_ll_session_begin_algo's / _sipp's
 * `workgroups` with (256 CUs x this; the SIPP kernel's LDS tier is fixed: 16 per CU).  The A*-epsilon-only kernels keep the tier's (time, cell) bitmap in device memory and take 8 KB less
 * LDS per search than the others, so the answer depends on the algorithm. */
int mrp_ll_session_occupancy(mrp_ll_ctx* ctx, int32_t algo, int32_t* occupancy_out);

/* Blocking: run n_jobs independent searches, fill results[i] for jobs[i]. */
int mrp_ll_search_batch(mrp_ll_ctx* ctx, int32_t n_jobs, const mrp_ll_job* jobs, mrp_ll_result* results);

/* Asynchronous form of the same call: submit returns a ticket; results are valid after mrp_ll_wait(ticket). */
int mrp_ll_submit(mrp_ll_ctx* ctx, int32_t n_jobs, const mrp_ll_job* jobs, mrp_ll_result* results, int32_t* ticket);
int mrp_ll_wait(mrp_ll_ctx* ctx, int32_t ticket);

/* ---- session mode -------------------------------------------------------------------------------------------
 * Between mrp_ll_session_begin and mrp_ll_session_end the context keeps `workgroups` wavefronts resident on the GPU
 * and feeds them through a job ring in pinned host memory: mrp_ll_submit publishes its jobs immediately (no launch,
 * no stream command) and returns MRP_LL_E_BUSY when the ring has no room for the whole batch (consume finished
 * tickets, then retry); mrp_ll_poll is the non-blocking form of mrp_ll_wait.  Searches of different tickets finish in
 * any order, so a caller can keep thousands of independent conflict trees moving without waiting for the slowest
 * search of a batch.  Results are identical to the batch mode's.
 * Liveness: the resident wavefronts watch a heartbeat that every mrp_ll_submit* / mrp_ll_poll* / mrp_ll_wait call
 * moves, and leave on their own only when it has stood still for 20 s (a caller that died); a caller that keeps
 * polling may pause between submits for as long as it likes.  If the resident kernel is gone while jobs are in flight
 * (that limit, or a device fault), mrp_ll_poll_any / mrp_ll_wait return MRP_LL_E_DEVICE instead of spinning. */
int mrp_ll_session_begin(mrp_ll_ctx* ctx, int32_t workgroups /* 0 = mrp_ll_options.slots */);
/* The same for MRP_LL_SIPP jobs (a session serves one kind: A* / A*-epsilon jobs, or SIPP jobs — the other kind comes
 * back as MRP_LL_BAD_JOB).  At most 512 SIPP jobs are in flight at a time (MRP_LL_E_BUSY beyond that). */
int mrp_ll_session_begin_sipp(mrp_ll_ctx* ctx, int32_t workgroups);
/* A session for jobs of ONE algorithm (MRP_LL_ASTAR, MRP_LL_ASTAR_EPS or MRP_LL_SIPP): the resident kernel is the one
 * specialised for it — half the code and fewer registers than the mixed kernel of mrp_ll_session_begin, same results;
 * jobs of another algorithm come back as MRP_LL_BAD_JOB.  What the conflict-tree drivers use. */
int mrp_ll_session_begin_algo(mrp_ll_ctx* ctx, int32_t algo, int32_t workgroups);
/* An MRP_LL_ASTAR_EPS session as a PAIR of resident launches: `workgroups` front workgroups that run every search in the
 * LDS tier (1023 open entries, 64 time steps) and nothing else, and `heavy_workgroups` heavy ones with a 31.4 KB window
 * (3071 open entries, as many time steps as the arena slot holds — 512 by default; the arena tier behind it) that take over — through a device-side queue, without the
 * host — the searches that outgrow it.  Same jobs, same results as mrp_ll_session_begin_algo; the split keeps the long
 * searches out of the many small windows and gives them an LDS-resident tier of their own.
 * workgroups + heavy_workgroups <= mrp_ll_options.slots (each needs an arena slot).  If the heavy workgroups do not become
 * resident (no room left on the device), the call falls back to mrp_ll_session_begin_algo's single launch.
 * heavy_workgroups = 0 is that call. */
int mrp_ll_session_begin_tiers(mrp_ll_ctx* ctx, int32_t algo, int32_t workgroups, int32_t heavy_workgroups);
/* The same for SEVERAL contexts that begin their sessions on one device at the same time (one per host thread): a heavy
 * workgroup needs 31.4 KB of one CU's LDS in one piece, which no CU has left once the front workgroups of another context
 * have spread over the device.  Every caller passes the same `gate` (zero before the first call) and `parties` (the number
 * of callers): each launches its heavy workgroups, waits until they run, arrives at the gate, and launches its front
 * workgroups only when all parties have arrived (or 2 s have passed).  gate == NULL: no waiting. */
int mrp_ll_session_begin_tiers_gated(mrp_ll_ctx* ctx, int32_t algo, int32_t workgroups, int32_t heavy_workgroups,
                                     int32_t* gate, int32_t parties);
/* Resident workgroups per CU of such a session's front kernel with the current tier limits, and the LDS bytes one heavy
 * workgroup takes: a caller sizes the pair with 256 CUs x (160 KiB - its share of heavy windows) / front window. */
int mrp_ll_session_tiers_geometry(mrp_ll_ctx* ctx, int32_t* front_occupancy_out, int32_t* front_lds_bytes_out,
                                  int32_t* heavy_lds_bytes_out);
/* Where the FRONT workgroups of such a pair keep the focal path table of a search.  in_memory = 0 (a new context): behind
 * the LDS window when it fits mrp_ll_configure_tiers' lds_path_bytes, which the window is then launched with.  in_memory != 0:
 * always in the workgroup's arena slot — the window is launched without a table (10 880 bytes for every agent count), the
 * search reads the two table rows of an expansion with two vector loads, and a root chain's table is bounded by the arena
 * slot's path area instead of lds_path_bytes.  mrp_ll_session_tiers_geometry then reports that window and what the runtime
 * grants for it; mrp_ll_session_occupancy, single-launch sessions, batches and the heavy workgroups are not affected.
 * Results never depend on it.  MRP_LL_E_BUSY while a batch or a session is in flight. */
int mrp_ll_session_front_tables(mrp_ll_ctx* ctx, int32_t in_memory);
int mrp_ll_session_end(mrp_ll_ctx* ctx);
/* Session mode: the same as mrp_ll_submit.  There is one device queue and it is first in, first out; which search
 * starts next is decided by the ORDER in which the caller publishes — keep the queue shallow (about two searches per
 * resident wavefront) and publish the searches of the longest dependent chains first, as the conflict-tree drivers do.
 * `lane` (0 or 1) is accepted for source compatibility with round 1's two-ring design and otherwise ignored. */
int mrp_ll_submit_lane(mrp_ll_ctx* ctx, int32_t lane, int32_t n_jobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                       int32_t* ticket);
int mrp_ll_poll(mrp_ll_ctx* ctx, int32_t ticket, int32_t* done);
/* Session mode only: collect every ticket that has completed since the last call (its results are filled in and the
 * ticket is released, exactly as after mrp_ll_wait).  One pass over the ring's completion words, independent of how
 * many tickets are in flight.  Writes at most `cap` ticket ids to `tickets`, their number to *n. */
int mrp_ll_poll_any(mrp_ll_ctx* ctx, int32_t* tickets, int32_t cap, int32_t* n);

/* Session mode, TWO host threads on one context ("co-workers": the device serves about twenty resident kernels of a
 * process well, a host core feeds about half a kernel's worth of conflict trees).  These two calls — and only these — may
 * be made concurrently by the co-workers of a context; session_begin / session_end / everything else stay with one of
 * them while the other is not inside a call.  `tag` (0 .. 3) names the caller: mrp_ll_poll_any_tagged hands out only the
 * tickets submitted under the same tag (it still unpacks every finished job it comes across into its caller's result
 * buffers, which must therefore stay valid until the ticket has been collected by its owner). */
int mrp_ll_submit_tagged(mrp_ll_ctx* ctx, int32_t tag, int32_t n_jobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                         int32_t* ticket);
int mrp_ll_poll_any_tagged(mrp_ll_ctx* ctx, int32_t tag, int32_t* tickets, int32_t cap, int32_t* n);

/* ---- high-level conflict scans -----------------------------------------------------------
 * Environment::getFirstConflict (example/ecbs.cpp:401-452, example/cbs.cpp identical) and Environment::focalHeuristic
 * (example/ecbs.cpp:315-350) for a batch of solutions (conflict-tree nodes) in one kernel launch.
 * Solution s owns agents set_first_agent[s] .. set_first_agent[s+1]-1 of the flattened agent list; agent a owns states
 * path_first_state[a] .. path_first_state[a+1]-1 of states_xy ([total][2] = x, y at time 0, 1, 2, ...; every path has
 * at least one state, coordinates 0..255).  out[s]: the first conflict in the reference's scan order (time ascending; at
 * one time step vertex pairs before edge pairs; pairs (i, j), i < j, lexicographic; the last time step is never
 * checked) and the number of all conflicts (= focalHeuristic). */
typedef struct mrp_ll_conflict {
  int32_t found;          /* getFirstConflict's return value                                                  */
  int32_t time;           /* Conflict::time                                                                   */
  int32_t agent1, agent2; /* Conflict::agent1 < Conflict::agent2 (indices inside the solution)                */
  int32_t type;           /* 0 = Conflict::Vertex, 1 = Conflict::Edge                                         */
  int32_t x1, y1, x2, y2; /* Vertex: the shared cell in x1, y1; Edge: agent1's move (x1,y1) -> (x2,y2)         */
  int32_t count;          /* focalHeuristic(solution)                                                         */
} mrp_ll_conflict;
int mrp_ll_conflict_scan(mrp_ll_ctx* ctx, int32_t n_sets, const int32_t* set_first_agent,
                         const int32_t* path_first_state, const int32_t* states_xy, mrp_ll_conflict* out);

/* The same scan for a conflict-tree CHILD, done by the workgroup that ran the child's low-level search: it holds every path
 * of the node (the focal context it built from the path store, and the path it has just found), so the node's conflicts
 * come back with the search instead of costing the caller a scan of its own — or, for a caller who keeps the node's paths
 * in the path store only, a trip of every path back to the host.
 * Submission: in a session exactly mrp_ll_submit_tagged (same lock, same tag rules; collected by mrp_ll_poll_any[_tagged] /
 * mrp_ll_poll / mrp_ll_wait); outside a session exactly mrp_ll_submit (`tag` is ignored; collected by mrp_ll_wait).
 * `conflicts` must stay valid as long as `results` must.  Jobs with and without MRP_LL_JOB_SCAN_CONFLICTS may share the
 * call; conflicts[i] of a job without the flag is not written.
 * A flagged job is valid only if: algo == MRP_LL_ASTAR_EPS; path_ids != NULL, a path store is reserved and the context is
 * accepted by id (the table-size limits of path_ids apply); n_agents >= 1 and 0 <= agent_idx < n_agents; every OTHER agent j
 * has path_ids[j] >= 0 and path_len[j] >= 1 (getState asserts a non-empty path, ecbs.cpp:491); no MRP_LL_JOB_ROOT_CHAIN;
 * and it came through THIS call — a flagged job sent through any other entry point is MRP_LL_BAD_JOB, like every other
 * invalid one, and is not run.
 * conflicts[i] of a flagged job that ends MRP_LL_OK or MRP_LL_PATH_TRUNCATED is exactly what mrp_ll_conflict_scan returns
 * for the solution S with S[agent_idx] = the path this search found (all of it, also when the caller's buffer was too
 * small) and S[j] = the path in slot path_ids[j]; agent numbers are indices into the job's n_agents.  With any other
 * status found = -1 and the other nine fields are 0.  The job's result — status, cost, fmin, n_states, expanded, path,
 * tier — is the same with and without the flag.  Works in batches and in every kind of A*-epsilon or mixed session; in a
 * mrp_ll_session_begin_tiers session the workgroup that FINISHES the search scans (a front workgroup that hands a search
 * over does not).  The scan is one wavefront's work, quadratic in the agents: about 12 000 ballots for 100 agents and 60
 * time steps. */
int mrp_ll_submit_scan(mrp_ll_ctx* ctx, int32_t tag, int32_t n_jobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                       mrp_ll_conflict* conflicts /* [n_jobs] */, int32_t* ticket);

/* ---- device-resident constraint store ------------------------------------------------------------------------
 * A conflict-tree child differs from its parent in one constraint (cbs.hpp:139-161, ecbs.hpp:243-270 copy the whole set and
 * add one).  With this store the agent's set stays on the device: the parent's search left it in a slot, the child's job
 * names that slot and ships only what it adds — instead of the whole set being scanned, re-encoded and written to pinned
 * host memory by the packer and read over PCIe by the workgroup for every job, O(tree depth) each.
 * n_slots sets of up to words_per_slot packed constraint words each (vertex + edge together).
 * words_per_slot <= 2048 (the union is assembled in the arena slot's copy area), else MRP_LL_E_INVALID.
 * MRP_LL_E_BUSY while a batch or a session is in flight; calling it again re-allocates (contents are lost);
 * n_slots == 0 frees the store.  mrp_ll_release_maps forgets every set (the slots stay allocated). */
int mrp_ll_constraint_store_reserve(mrp_ll_ctx* ctx, int32_t n_slots, int32_t words_per_slot);

typedef struct mrp_ll_constraint_ref {
  int32_t base_set_id;    /* -1: none; else the set this job's agent has at the PARENT node */
  int32_t result_set_id;  /* -1: none; else the slot that receives  base + the job's own constraint arrays */
} mrp_ll_constraint_ref;

#define MRP_LL_JOB_CONSTRAINT_SET 32   /* mrp_ll_job.flags: sets[i] of mrp_ll_submit_sets is honoured for this job */

/* mrp_ll_submit_scan plus `sets`; conflicts may be NULL when no job has MRP_LL_JOB_SCAN_CONFLICTS, sets may be NULL when no
 * job has MRP_LL_JOB_CONSTRAINT_SET.  Same lock, tag rules and collection calls as mrp_ll_submit_scan, in and outside a
 * session.
 * The set a flagged job's search sees is the contents of base_set_id, if any, followed by the job's vertex_constraints /
 * edge_constraints — now the ADDITIONS, typically one or none; with result_set_id >= 0 that union is left in the slot for
 * later jobs to name (whenever the job ran, whatever its status).  Every field of the result — status, cost, fmin, n_states,
 * expanded, path, tier, a scan's conflicts — is exactly what the same job returns with the whole union shipped in its
 * arrays.  Nothing is de-duplicated: a constraint added twice costs a word and changes no result.  An unflagged job of the
 * same call ignores sets[i]: a zero-initialised job touches no slot.
 * A set belongs to the map and the goal cell of the job that wrote it (m_lastGoalConstraint, ecbs.cpp:268-273, is kept with
 * the set).  Slot ids are the caller's to hand out; a slot may be reused once no unfinished job names it.
 * A flagged job comes back MRP_LL_BAD_JOB, not run and with no set created or changed, when: no store is reserved; an id is
 * out of range; the base was never written, or the ticket of the job that writes it has not been collected yet; the base
 * belongs to another map or another goal cell; base_set_id == result_set_id; the union exceeds words_per_slot; algo is not
 * MRP_LL_ASTAR or MRP_LL_ASTAR_EPS; MRP_LL_JOB_ROOT_CHAIN is set; or it came through any other entry point. */
int mrp_ll_submit_sets(mrp_ll_ctx* ctx, int32_t tag, int32_t n_jobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                       mrp_ll_conflict* conflicts, const mrp_ll_constraint_ref* sets, int32_t* ticket);

/* ---- a conflict-tree child's conflicts from what its PARENT's scan established ---------------------------------
 * A child differs from its parent in one path, and the caller that scanned the parent knows its number of conflicts and a
 * time before which it has none (the time of the conflict it was split on; ecbs.hpp:200-270).  Given both and the slot of
 * the REPLACED path, the workgroup produces the child's mrp_ll_conflict with work linear in the agents for the count and
 * all-pairs work only for the time steps between the parent's first conflict and the child's, instead of
 * MRP_LL_JOB_SCAN_CONFLICTS' all pairs at every time step. */
typedef struct mrp_ll_scan_base {
  int32_t parent_count;   /* focalHeuristic of the PARENT node (agent_idx's replaced path in place) */
  int32_t clean_before;   /* the parent node has no conflict at any time step < this; 0 is always valid */
} mrp_ll_scan_base;

#define MRP_LL_JOB_SCAN_FROM_PARENT 64 /* mrp_ll_job.flags, only together with MRP_LL_JOB_SCAN_CONFLICTS: bases[i] of
                                        * mrp_ll_submit_node is honoured for this job */

/* mrp_ll_submit_sets plus `bases`; bases may be NULL when no job has MRP_LL_JOB_SCAN_FROM_PARENT, and an unflagged job
 * ignores bases[i].  Same lock, tag rules and collection calls as mrp_ll_submit_sets, in and outside a session.
 * A flagged job must satisfy everything MRP_LL_JOB_SCAN_CONFLICTS requires; in addition path_ids[agent_idx] >= 0 names the
 * path-store slot of the replaced path — agent_idx's path at the parent node — with path_len[agent_idx] >= 1 (the search
 * still never sees its own agent's column: the slot is not part of the focal context), and parent_count >= 0,
 * clean_before >= 0.  Anything else, the flag without MRP_LL_JOB_SCAN_CONFLICTS, or the flag through any other entry point,
 * is MRP_LL_BAD_JOB: not run, no slot touched.
 * With a = agent_idx, tPad = the longest other path, L_new = the found path's length, L_old = the length stored in the
 * replaced path's slot, T_x = max(tPad, L_x) - 1 and C(p, T) = the vertex + swap conflicts between path p and every other
 * agent at t < T (every path holding its last cell beyond its end):  T_new == T_old gives
 * count = parent_count - C(old, T) + C(new, T); with different horizons the workgroup runs MRP_LL_JOB_SCAN_CONFLICTS' full scan
 * (stationary agents that share a last cell make the extra steps count).  found and the first conflict are the child's, in
 * mrp_ll_conflict_scan's order.  With TRUTHFUL bases all ten words of conflicts[i] equal mrp_ll_conflict_scan of the
 * child, which is also what the same job returns with MRP_LL_JOB_SCAN_CONFLICTS alone; the job's result never depends on
 * the flag; a status other than MRP_LL_OK / MRP_LL_PATH_TRUNCATED gives found = -1, the rest 0; n_agents == 1 gives found 0,
 * count 0.
 * UNTRUTHFUL bases (a wrong parent_count, a clean_before behind the parent's first conflict, a slot that holds another
 * path) give a wrong mrp_ll_conflict and nothing else: no access outside the job's buffers, no loop beyond T time steps. */
int mrp_ll_submit_node(mrp_ll_ctx* ctx, int32_t tag, int32_t n_jobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                       mrp_ll_conflict* conflicts, const mrp_ll_constraint_ref* sets, const mrp_ll_scan_base* bases /* [n_jobs] */,
                       int32_t* ticket);

/* ---- the root node of a CBS-TA conflict tree -------------------------------------------------------------------
 * CBS with task assignment plans a whole new root for every popped root that still has a conflict (cbs_ta.hpp:142-172): n
 * unconstrained low-level searches under the next-best assignment, then Environment::getFirstConflict over their paths.
 * Here ONE workgroup does that for one root and a batch of roots is ONE kernel launch that ends (workgroup b takes roots
 * b, b + grid, ...; grid = min(n_roots, mrp_ll_options.slots)): no job descriptor and no result round trip per agent, no
 * scan on the host.
 * Agents are planned in index order, each with no constraints; agent a's search is exactly the one the ordinary
 * MRP_LL_ASTAR_TA job {map_id, start = starts_xy[a], goal = goals_xy[a], heuristic_id = heuristic_ids[a], or
 * MRP_LL_JOB_NO_GOAL where heuristic_ids[a] < 0} runs — the LDS tier where it fits, the arena tier otherwise — and
 * results[a] is field for field what that job returns: status, cost, fmin, n_states, expanded, tier, states, actions,
 * action costs (MRP_LL_PATH_TRUNCATED included; the root still counts such an agent as planned).
 * The root ends BEHIND the first agent whose search does not end MRP_LL_OK (the break at cbs_ta.hpp:159-162): later agents
 * come back MRP_LL_NOT_RUN with cost, fmin, n_states, expanded and tier 0; planned[r] = results filled in.
 * max_expansions is the budget of the whole root, shared as a root chain's (MRP_LL_JOB_ROOT_CHAIN): each search gets what
 * the ones before it left; an empty budget starts the next search with 0, which comes back MRP_LL_CAP_EXPANSIONS with
 * expanded = 1.
 * conflicts[r]: when every agent got a path, exactly what mrp_ll_conflict_scan returns for those n_agents paths; otherwise
 * found = -1 and the other nine fields 0.  The workgroup keeps the paths as a time-major table of  longest path x (n_agents
 * rounded up to 16) x 2  bytes in its arena slot's path area (128 KiB by default: room for 64 agents and 1024 time steps)
 * and scans it there; a table beyond that area is not built, and the call completes conflicts[r] with the batch scan
 * of mrp_ll_conflict_scan on the paths it holds before it returns — the caller always receives the answer.
 * A root is refused on the host, with nothing run for it and the other roots unaffected — planned[r] = 0, every result
 * MRP_LL_BAD_JOB, found = -1 — when: map_id is unknown; a start lies outside the grid; a heuristic id is unknown or belongs
 * to another map, or its goal lies outside the grid (what makes the ordinary job MRP_LL_BAD_JOB); n_agents is outside
 * 1 .. 64; starts_xy, goals_xy, heuristic_ids or results is NULL.
 * The refusal is written to results[0 .. n_agents - 1] as the caller counted them, also for a count above 64: `results`
 * must hold n_agents entries whenever it is not NULL and n_agents is positive.
 * MRP_LL_E_INVALID: a NULL argument, n_roots < 0.  MRP_LL_E_BUSY while a session is active or a batch is in flight, like
 * the assignment calls.  n_roots == 0 succeeds without a launch.
 * On MRP_LL_E_DEVICE / MRP_LL_E_NOMEM (a launch, an allocation or the completing scan failed) the outputs say that nothing
 * ran, never half of it: planned[r] = 0 and found = -1 for every root, every result of a root that would have been refused
 * MRP_LL_BAD_JOB and of every other root MRP_LL_NOT_RUN, their other fields 0.
 * Tuning knob: the environment variable MRP_LL_ARENA_PATHS_BYTES, read by mrp_ll_create, sets the path area of every arena
 * slot of the contexts created under it (4096 .. 131072 bytes, rounded down to a multiple of 256; unset: 131072).  The area
 * is shared: it also holds the focal table of an A*-epsilon job that does not fit LDS, a root chain's table in a
 * mrp_ll_session_front_tables session and the travelling safe-interval table of a SIPP job, so under a smaller value jobs
 * with larger tables come back MRP_LL_BAD_JOB (path_ids tables, root chains) or are read from host memory (shipped tables)
 * that a default context serves from the slot.  Results never depend on it; it exists for tests and measurements. */
typedef struct mrp_ll_ta_root {
  int32_t map_id, n_agents;        /* 1 .. 64 (the narrow assignment's limit); the _w calls: 1 .. 256 */
  const int32_t* starts_xy;        /* [n_agents][2] */
  const int32_t* goals_xy;         /* [n_agents][2]; ignored where heuristic_ids[a] < 0 */
  const int32_t* heuristic_ids;    /* [n_agents]; < 0: the agent has no task (MRP_LL_JOB_NO_GOAL) */
  int64_t max_expansions;          /* budget of the whole root, < 0 unlimited */
  mrp_ll_result* results;          /* [n_agents], each with its own caller buffers */
} mrp_ll_ta_root;
int mrp_ll_ta_root_batch(mrp_ll_ctx* ctx, int32_t n_roots, const mrp_ll_ta_root* roots, int32_t* planned /* [n_roots] */,
                         mrp_ll_conflict* conflicts /* [n_roots] */);

/* ---- the root node of an ECBS-TA conflict tree ------------------------------------------------------------------
 * ECBS with task assignment plans a root agent after agent (ecbs_ta.hpp:117-138, :306-343): agent a's AStarEpsilon search
 * under weight w has no constraints and sees the paths of agents 0 .. a - 1 as its focal context; then
 * Environment::focalHeuristic counts the conflicts of the n paths.  As with mrp_ll_ta_root_batch ONE workgroup does that for
 * one root, and a batch of roots is ONE kernel launch that ends (mrp_ll_ta_eps_root_kernel).  The roots are mrp_ll_ta_root
 * records; what is said there holds here, with these differences:
 * results[a] is field for field what the ordinary MRP_LL_ASTAR_EPS_TA job {map_id, w, agent_idx = a, start, goal,
 * heuristic_id or MRP_LL_JOB_NO_GOAL, no constraints, n_agents, and as shipped context the paths of agents 0 .. a - 1, the
 * others empty} returns — fmin included, whose sum is the node's LB.
 * conflicts[r].count is the node's focalHeuristic (ecbs_ta.cpp:347-382).
 * The workgroup keeps ONE time-major table in its arena slot's path area: the focal context of the next search and the
 * scan's input.  If a path would make the table outgrow the area (only under MRP_LL_ARENA_PATHS_BYTES: by default 64 agents
 * x 1024 steps fit), the kernel stops behind that agent and the CALL completes the root before it returns — the remaining
 * agents as ordinary jobs with shipped contexts, one after the other under what is left of the budget, and the scan by
 * mrp_ll_conflict_scan.  The caller always receives the same answer.
 * MRP_LL_E_INVALID also for w < 1 or NaN. */
int mrp_ll_ta_eps_root_batch(mrp_ll_ctx* ctx, float w, int32_t n_roots, const mrp_ll_ta_root* roots,
                             mrp_ll_conflict* conflicts /* [n_roots] */, int32_t* planned /* [n_roots] */);

/* The same call for a caller that keeps its paths in the device-resident path store (mrp_ll_path_store_reserve):
 * result_path_ids[r][a] >= 0 is the slot that ALSO receives the path of agent a of root r, exactly as
 * MRP_LL_JOB_STORE_RESULT does for an ordinary job, so that the children of the root can name it (mrp_ll_job.path_ids); -1 =
 * not stored.  result_path_ids == NULL, or result_path_ids[r] == NULL, stores nothing: mrp_ll_ta_eps_root_batch is this call
 * with NULL.  Results, planned and conflicts are bit for bit what the call without ids returns.  Only the slots of agents that
 * come back MRP_LL_OK are written; the slot of any other agent (not planned, no path) keeps its content.  The agents the call
 * completes on the host (above) store their paths too.  A root with an id below -1 or outside the reserved store is refused
 * like any other invalid root: MRP_LL_BAD_JOB in each of its results, nothing run, no slot touched. */
int mrp_ll_ta_eps_root_batch_stored(mrp_ll_ctx* ctx, float w, int32_t n_roots, const mrp_ll_ta_root* roots,
                                    mrp_ll_conflict* conflicts /* [n_roots] */, int32_t* planned /* [n_roots] */,
                                    const int32_t* const* result_path_ids /* [n_roots] -> [n_agents]; NULL = none */);

/* ---- the same roots with up to 256 agents -------------------------------------------------------------------------
 * mrp_ll_ta_root_batch_w and mrp_ll_ta_eps_root_batch_w are mrp_ll_ta_root_batch and mrp_ll_ta_eps_root_batch for roots of
 * 1 .. 256 agents (what mrp_ll_assign_series_create_w assigns): the same records, refusals (with 256 in place of 64), one
 * budget per root, MRP_LL_NOT_RUN, planned, ten conflict words, return codes and MRP_LL_E_BUSY, word for word.  Still ONE
 * workgroup per root and ONE launch per call.  The four root kernels are one source (csrc/ll_ta_root.h, a template over the
 * algorithm and the agents per lane): mrp_ll_ta_root_wide_kernel and mrp_ll_ta_eps_root_wide_kernel keep four agents in each
 * lane, the narrow calls' kernels one, and the narrow calls go on
 * refusing 65 agents.  A root of at most 64 agents gets from a _w call exactly what the narrow call returns.
 * The table of a root is  longest path x (n_agents rounded up to 16) x 2  bytes: 256 agents fill the default path area of
 * 128 KiB at 256 time steps.  Beyond it the narrow calls' fall-backs apply unchanged: the CBS-TA call completes the scan with
 * mrp_ll_conflict_scan, the ECBS-TA call plans the remaining agents as ordinary jobs with shipped contexts and scans.
 * There is no path-store variant of the wide ECBS-TA call. */
int mrp_ll_ta_root_batch_w(mrp_ll_ctx* ctx, int32_t n_roots, const mrp_ll_ta_root* roots, int32_t* planned /* [n_roots] */,
                           mrp_ll_conflict* conflicts /* [n_roots] */);
int mrp_ll_ta_eps_root_batch_w(mrp_ll_ctx* ctx, float w, int32_t n_roots, const mrp_ll_ta_root* roots,
                               mrp_ll_conflict* conflicts /* [n_roots] */, int32_t* planned /* [n_roots] */);

int mrp_ll_get_stats(const mrp_ll_ctx* ctx, mrp_ll_stats* out);
int mrp_ll_reset_stats(mrp_ll_ctx* ctx);

/* Library version / build info ("gfx950 ..."). */
const char* mrp_ll_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MRP_LL_H */
