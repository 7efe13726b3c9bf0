/*
 * mrp_hl.h — host-side conflict-tree drivers (libmrp_hl.so) that CALL the low-level C-ABI of mrp_ll.h.
 *
 * These are the callers of the hot path, restated so that many MAPF instances advance in lock-step and every round
 * hands ALL ready low-level searches to the GPU in one mrp_ll_submit:
 *   CBS::search   include/libMultiRobotPlanning/cbs.hpp:85-172   (root: N independent searches; then 2 per CT node)
 *   ECBS::search  include/libMultiRobotPlanning/ecbs.hpp:109-288 (root: chain of N searches, each seeing the paths
 *                 planned so far; then 2 per CT node; HL open by cost, HL focal by (focalHeuristic, cost))
 * with the HL-side Environment methods of example/ecbs.cpp: getFirstConflict :401-452, createConstraintsFromConflict
 * :454-472, focalHeuristic :315-350.  The high-level heaps replay boost::heap::d_ary_heap exactly (tie order decides
 * which CT node is expanded), so cost / makespan / highLevelExpanded / lowLevelExpanded equal the reference's
 * `statistics:` block (example/ecbs.cpp:594-599) — checked against the oracle in tests/.
 *
 * Also here: the seeded synthetic-instance generator used by bench.py and the YAML subset
 * reader / schedule writer of example/ecbs.cpp:554-574,584-617.
 */
#ifndef MRP_HL_H
#define MRP_HL_H

#include <stdint.h>

#include "mrp_ll.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRP_HL_CBS 0
#define MRP_HL_ECBS 1

/* mrp_hl_solution.status */
#define MRP_HL_SOLVED 0       /* search() returned true                                                        */
#define MRP_HL_NO_SOLUTION 1  /* search() returned false (a root search failed or the CT open list ran empty)   */
#define MRP_HL_CAP 2          /* a harness cap was hit (the reference has none and would keep running)          */
#define MRP_HL_LL_ERROR 3     /* a low-level job came back with a capacity status (MRP_LL_CAP_NODES/HORIZON/..) */

typedef struct mrp_hl_instance {
  int32_t dimx, dimy;
  int32_t n_obstacles;
  const int32_t* obstacles_xy; /* [n][2]  (map.obstacles, ecbs.cpp:564-566) */
  int32_t n_agents;
  const int32_t* starts_xy;    /* [n][2]  (agents[].start, ecbs.cpp:571)     */
  const int32_t* goals_xy;     /* [n][2]  (agents[].goal,  ecbs.cpp:573)     */
} mrp_hl_instance;

typedef struct mrp_hl_solution {
  int32_t status;
  int32_t n_ll_searches;          /* low-level searches issued for this instance                                */
  int64_t cost;                   /* statistics.cost      (sum of PlanResult::cost, ecbs.cpp:586-591)            */
  int64_t makespan;               /* statistics.makespan                                                        */
  int64_t high_level_expanded;    /* statistics.highLevelExpanded                                               */
  int64_t low_level_expanded;     /* statistics.lowLevelExpanded  (the metric's numerator)                      */
  int32_t* path_len;              /* caller buffer [n_agents] or NULL                                           */
  int32_t* paths_xy;              /* caller buffer [n_agents][path_cap][2] or NULL                              */
  int32_t path_cap;
  int32_t reserved;
  /* FNV-1a (64 bit) of the schedule of a SOLVED instance — for every agent in order: the bytes x, y of every state of its
   * path, then the byte 0xFF — computed from the full paths whether or not paths_xy holds (all of) them: a caller that
   * checks a million schedules compares eight bytes each.  0 when status != MRP_HL_SOLVED. */
  uint64_t schedule_digest;
} mrp_hl_solution;

typedef struct mrp_hl_options {
  int32_t algo;                   /* MRP_HL_CBS | MRP_HL_ECBS                                                    */
  float w;                        /* ECBS suboptimality bound (binary32, ecbs.cpp:530,536)                        */
  int64_t max_ll_expansions;      /* per instance, summed over its searches; < 0 unlimited                        */
  int64_t max_hl_expansions;      /* per instance; < 0 unlimited                                                  */
  int32_t n_threads;              /* host worker threads == instance groups in flight (0 = default)               */
  int32_t mode;                   /* 0 = session (resident kernel, every instance advances on its own; default),   */
                                  /* 1 = rounds (one launch per round of ready searches; simpler, slower)          */
} mrp_hl_options;

typedef struct mrp_hl_batch_stats {
  double wall_seconds;            /* timed region: all conflict-tree searches of the batch, first submit to last result */
  int64_t rounds;                 /* mrp_ll_submit calls                                                          */
  int64_t ll_searches;
  int64_t ll_expansions;          /* of the searches the conflict trees consumed (== sum of solutions' low_level_expanded) */
  int64_t solved;
  /* host-side time summed over worker threads (diagnostic): building jobs, inside mrp_ll_search_batch, consuming results */
  double build_seconds, ll_call_seconds, consume_seconds;
  /* look-ahead of the conflict-tree machines (session mode; MRP_HL_SPEC): searches issued before their CT node was popped,
   * and the expansions of searches that were run but whose node was never popped (work, not part of ll_expansions) */
  int64_t speculative_searches, wasted_ll_expansions;
  /* ECBS sessions: instances whose root node had no conflict — found by the workgroup that ran the root chain
   * (mrp_ll.h MRP_LL_JOB_ROOT_CHAIN) — and whose solution was written without a conflict-tree object */
  int64_t root_solved;
  /* ECBS sessions with MRP_HL_DEVICE_SCAN=1: conflict-tree nodes whose first conflict and conflict count came back with their
   * low-level search (mrp_ll.h mrp_ll_submit_scan) instead of being scanned by the driver; 0 otherwise */
  int64_t device_scans;
  /* ... those of them (MRP_HL_DEVICE_SCAN_INCREMENTAL=1, an engine with mrp_ll_submit_node) whose workgroup started from what
   * the parent node's scan had established (MRP_LL_JOB_SCAN_FROM_PARENT); counted in device_scans too; 0 otherwise */
  int64_t incremental_scans;
} mrp_hl_batch_stats;

/* One engine context per calling thread is created internally for every worker thread on `device`. */
int mrp_hl_solve_batch(int32_t device, const mrp_hl_options* opt, int32_t n_instances, const mrp_hl_instance* instances,
                       mrp_hl_solution* solutions, mrp_hl_batch_stats* stats);

/* mrp_hl_solve_batch with the true grid distance to the goal as the low-level heuristic (what example/cbs.cpp:445-557 carries
 * switched off): the same contract, instances, options, solutions and statistics, but every low-level search of every conflict
 * tree goes out with MRP_LL_JOB_TABLE_H (mrp_ll.h) and the shortest-path table of its agent's goal.  The call uploads the maps
 * and computes one table per agent's goal with a single mrp_ll_compute_heuristics per engine, all BEFORE the timed region
 * (stats->wall_seconds), as the reference builds its Environment before it starts its Timer.  It runs in the rounds
 * schedule whatever opt->mode says: the session schedule opens one-algorithm sessions, which take no such job.
 * What changes against mrp_hl_solve_batch: the searches' expansion counts and, where several paths of equal cost exist, the
 * paths; CBS's cost (the optimum) does not, ECBS's stays within w of it.  The look-ahead, root-chain, device-scan and store
 * knobs of the session schedule do not apply.
 * MRP_LL_E_NOMEM: the tables do not fit the engines' maps buffer — the call fails with a message on stderr; it never falls back
 * to the Manhattan searches. */
int mrp_hl_solve_batch_table_h(int32_t device, const mrp_hl_options* opt, int32_t n_instances,
                               const mrp_hl_instance* instances, mrp_hl_solution* solutions, mrp_hl_batch_stats* stats);

/* Persistent form for benchmarking: engines (and their arenas) are created once and reused across batches. */
typedef struct mrp_hl_solver mrp_hl_solver;
int mrp_hl_solver_create(int32_t device, int32_t n_threads, const mrp_ll_options* ll_opt, mrp_hl_solver** out);
void mrp_hl_solver_destroy(mrp_hl_solver* s);
int mrp_hl_solver_solve(mrp_hl_solver* s, const mrp_hl_options* opt, int32_t n_instances,
                        const mrp_hl_instance* instances, mrp_hl_solution* solutions, mrp_hl_batch_stats* stats);
/* Two-step form: preload uploads the instances' static maps to HBM (the reference builds its Environment before it
 * starts its Timer, example/ecbs.cpp:576-582) and fixes the instance -> worker assignment; solve_preloaded then runs the
 * conflict-tree searches only.  The instance arrays must stay valid until mrp_hl_preloaded_free. */
typedef struct mrp_hl_preloaded mrp_hl_preloaded;
int mrp_hl_solver_preload(mrp_hl_solver* s, int32_t n_threads, int32_t n_instances, const mrp_hl_instance* instances,
                          mrp_hl_preloaded** out);
int mrp_hl_solver_solve_preloaded(mrp_hl_solver* s, const mrp_hl_options* opt, mrp_hl_preloaded* p,
                                  mrp_hl_solution* solutions, mrp_hl_batch_stats* stats);
/* Several preloaded batches (of this solver, preloaded with the same n_threads) as ONE stream: the worker threads draw
 * batch 0's instances, then batch 1's, ... from one pool with no barrier between batches, so the dependent chains that end
 * a batch — deep conflict trees (ecbs.hpp:151-285 is a sequential loop per instance), searches that run to the harness cap —
 * overlap with the root searches of the next batch instead of leaving the device idle.  Instances are independent
 * (one conflict tree each), so solutions[b][k] is exactly what mrp_hl_solver_solve_preloaded(batches[b]) writes; `stats`
 * is the aggregate over the stream (wall_seconds: the whole call).  n_batches = 1 is mrp_hl_solver_solve_preloaded.
 * Several batches need the session driver (mrp_hl_options.mode 0). */
int mrp_hl_solver_solve_stream(mrp_hl_solver* s, const mrp_hl_options* opt, int32_t n_batches,
                               mrp_hl_preloaded* const* batches, mrp_hl_solution* const* solutions,
                               mrp_hl_batch_stats* stats);
void mrp_hl_preloaded_free(mrp_hl_preloaded* p);
int mrp_hl_solver_ll_stats(mrp_hl_solver* s, mrp_ll_stats* out, int32_t reset); /* summed over its engines */
const char* mrp_hl_solver_last_error(const mrp_hl_solver* s);

/* Prioritized planning with SIPP (example/mapf_prioritized_sipp.cpp:214-270): agents are planned one after the other,
 * each against the collision intervals left by the agents before it; an agent that cannot be planned is skipped.
 * Every round plans the next agent of ALL instances in one MRP_LL_SIPP batch.
 * Per instance: cost = statistics.cost (sum over planned agents); planned[a] in {0,1}; n_states[a];
 * states_xyt [n_agents][state_cap][3] = x, y, t (the schedule the reference writes, :256-260). */
typedef struct mrp_hl_sipp_solution {
  int64_t cost;
  int64_t low_level_expanded;
  int32_t n_planned;
  int32_t status;       /* 0: every agent got the reference's answer (planned or "not found"); otherwise the MRP_LL_*
                         * capacity status (expansion cap, node arena, horizon) of the search that stopped THIS
                         * instance — its later agents are not planned; other instances of the batch are unaffected */
  int32_t* planned;     /* caller buffer [n_agents] */
  int32_t* n_states;    /* caller buffer [n_agents] */
  int32_t* states_xyt;  /* caller buffer [n_agents][state_cap][3] or NULL */
  int32_t state_cap;
  int32_t reserved2;
} mrp_hl_sipp_solution;
int mrp_hl_solver_prioritized_sipp(mrp_hl_solver* s, int32_t n_instances, const mrp_hl_instance* instances,
                                   mrp_hl_sipp_solution* solutions, mrp_hl_batch_stats* stats);

/* ---- one conflict tree, stepped by the caller ------------------------------------------------------------------
 * The same state machine the batch drivers run (CBS::search cbs.hpp:85-172 / ECBS::search ecbs.hpp:109-288 cut at the
 * low-level calls), exposed so that a caller can decide WHERE each low-level search runs — e.g. the searches of one
 * round sharded over several GPUs (libmultirobotplanning_amd/ct_sharded.py).  Pending requests come in
 * groups (the root step, or the two children of one conflict-tree node; with spec_width > 1 also the children of the
 * nodes that will probably be popped next); a group is answered as a whole, groups in any order.  The result of an
 * instance that is SOLVED (or has no solution) does not depend on spec_width or on the order of delivery.  An instance
 * that ends in MRP_HL_CAP reports MRP_HL_CAP either way, but its low_level_expanded / n_ll_searches may differ with
 * spec_width: a pre-computed search is issued with the budget left at that moment, before the searches in front of
 * it have been accounted. */
typedef struct mrp_hl_ct mrp_hl_ct;
int mrp_hl_ct_create(const mrp_hl_instance* instance, const mrp_hl_options* opt, int32_t map_id, int32_t spec_width,
                     mrp_hl_ct** out);
void mrp_hl_ct_destroy(mrp_hl_ct* ct);
int32_t mrp_hl_ct_n_requests(const mrp_hl_ct* ct);
/* Request k as a low-level job (map_id as given to create; its arrays stay valid until the next mrp_hl_ct_deliver). */
int mrp_hl_ct_request(const mrp_hl_ct* ct, int32_t k, mrp_ll_job* job, int32_t* group, int32_t* slot);
/* The results of every request of `group`, in slot order (status, cost, fmin, expanded, n_states, states_txy). */
int mrp_hl_ct_deliver(mrp_hl_ct* ct, int32_t group, int32_t n, const mrp_ll_result* results);
int32_t mrp_hl_ct_done(const mrp_hl_ct* ct);
int mrp_hl_ct_solution(const mrp_hl_ct* ct, mrp_hl_solution* out);

/* One round of a conflict tree whose searches are sharded over `world` ranks (ct_sharded.py): every rank
 * holds the same tree, group j of the pending requests belongs to rank j % world.
 *   mrp_hl_ct_round_mine   runs THIS rank's requests on `ll` (mrp_ll_search_batch) and packs their results into `rows`, one
 *                          row of 8 + max_states int32 words per search:
 *                            group, slot, status, cost, fmin, expanded (low 31 bits), expanded >> 31, n_states,
 *                            then one word x | y << 16 per state.
 *                          rows_per_rank[world] receives how many rows every rank produces this round (the same on all
 *                          ranks: the shape of the all-gather); returns the number of rows written (<= cap_rows), or
 *                          a negative MRP_LL_E_* — in which case the rank still writes ONE row with group = INT32_MIN, so that
 *                          the collective can take place and every rank sees the failure.
 *   mrp_hl_ct_deliver_rows takes the gathered rows of all ranks ([world][rows_stride][8 + max_states]) and delivers the
 *                          groups in their pending order.  MRP_LL_E_DEVICE if any rank reported a failure. */
int32_t mrp_hl_ct_round_mine(mrp_hl_ct* ct, mrp_ll_ctx* ll, int32_t rank, int32_t world, int32_t max_states, int32_t* rows,
                             int32_t cap_rows, int32_t* rows_per_rank);
int mrp_hl_ct_deliver_rows(mrp_hl_ct* ct, const int32_t* gathered, int32_t world, int32_t rows_stride, int32_t max_states);

/* ---- CBS with task assignment (cbs_ta.hpp:87-214 over the Environment of example/cbs_ta.cpp), batched --------------------
 * Every instance is a resumable state machine; every ROUND makes three device calls over all instances at once:
 * mrp_ll_assign_series_next for the instances that need a root (Environment::nextTaskAssignment, cbs_ta.cpp:442-456),
 * mrp_ll_ta_root_batch for the new roots (cbs_ta.hpp:98-116,142-172), mrp_ll_search_batch for the two child searches of every
 * popped node with a conflict (cbs_ta.hpp:179-210).  Before the first round: one mrp_ll_compute_heuristics launch for all
 * goals of all instances and one mrp_ll_assign_series_create (gather form; an agent may take only its own potential goals,
 * cbs_ta.cpp:272-280).
 * Tasks are the distinct potential goal cells in order of first appearance in the input (the reference iterates
 * unordered_sets: its order is unspecified); a potential goal outside the grid can never be assigned and is dropped.
 * The open list is ordered by cost alone and replays boost's d_ary_heap (hl/exact_heap.hpp).  A popped root with a conflict
 * first gets its new root — which takes `id`, advanced only when every agent got a path, and is pushed BEFORE the two
 * children; the expansions of a failed root count.  Conflicts are Environment::getFirstConflict's of cbs_ta.cpp:369-420, which
 * also looks at the time step at which the longest path ends (mrp_ll_conflict_scan does not: the driver adds that step).
 * Instances within 64 agents x 64 tasks share ONE mrp_ll_assign_series_create, the others ONE mrp_ll_assign_series_create_w;
 * all series advance in the round's one mrp_ll_assign_series_next.  With use_root_kernel = 1 the roots of at most 64 agents go
 * through mrp_ll_ta_root_batch and the others through mrp_ll_ta_root_batch_w: at most two root calls per round.
 * The cost is the reference's; among assignments of equal cost the series' documented order (cost, then creation number)
 * stands in for Boost's accidental one, so WHICH of several optimal solutions comes back is this project's own choice.
 * Limits: at most 256 agents and 256 tasks (distinct potential goals) per instance, assignment costs below 2^24 (the wide
 * assignment calls'); beyond them the instance ends MRP_HL_LL_ERROR, the other instances of the batch unaffected, as it does when a search comes back with a capacity status other than the expansion cap. */
typedef struct mrp_hl_ta_instance {
  int32_t dimx, dimy;
  int32_t n_obstacles;
  const int32_t* obstacles_xy;  /* [n][2] */
  int32_t n_agents;
  const int32_t* starts_xy;     /* [n_agents][2] */
  const int32_t* goal_first;    /* [n_agents + 1]: agent a's potential goals are goals_xy[goal_first[a] .. goal_first[a + 1]) */
  const int32_t* goals_xy;      /* [goal_first[n_agents]][2]  (agents[].potentialGoals, cbs_ta.cpp:560-566) */
} mrp_hl_ta_instance;

typedef struct mrp_hl_ta_options {
  int32_t max_task_assignments; /* m_maxTaskAssignments: no further assignment is asked for once MORE than this many non-empty */
                                /* ones have been handed out (the `>` of cbs_ta.cpp:443)                                          */
  int32_t use_root_kernel;      /* 1: roots through mrp_ll_ta_root_batch; 0: a root is n ordinary jobs inside the round's batch  */
                                /* and the driver's own scan.  Same results.  0 is the default of a NULL options pointer and of   */
                                /* the Python and CLI front-ends: measured faster at the reference shape    */
  int64_t max_hl_expansions;    /* per instance, < 0 unlimited: one more pop ends the instance MRP_HL_CAP                         */
  int64_t max_ll_expansions;    /* per instance, summed over its searches, < 0 unlimited -> MRP_HL_CAP; every search of a round   */
                                /* is issued with what was left when the round began, so the counters of a CAPPED instance may    */
                                /* differ between use_root_kernel 0 and 1                                                        */
} mrp_hl_ta_options;

typedef struct mrp_hl_ta_solution {
  int32_t status;               /* MRP_HL_SOLVED | MRP_HL_NO_SOLUTION (empty first assignment, failed first root, open list empty) */
                                /* | MRP_HL_CAP | MRP_HL_LL_ERROR                                                                */
  int32_t n_ll_searches;
  int64_t cost;                 /* statistics.cost (cbs_ta.cpp:582-587) */
  int64_t makespan;             /* statistics.makespan: the largest path COST */
  int64_t high_level_expanded;
  int64_t low_level_expanded;
  int64_t num_task_assignments; /* statistics.numTaskAssignments */
  int32_t n_roots;              /* roots pushed to the open list (diagnostic) */
  int32_t root_conflicts;       /* popped roots that had a conflict (diagnostic) */
  int32_t* task_xy;             /* caller buffer [n_agents][2] or NULL: the task of every agent of the solution, -1, -1 = none */
  int32_t* path_len;            /* caller buffer [n_agents] or NULL */
  int32_t* paths_xyt;           /* caller buffer [n_agents][path_cap][3] or NULL: x, y and the t the reference writes, which is */
                                /* the path's cost up to that state (cbs_ta.cpp:606-610), not its index                          */
  int32_t path_cap;
  int32_t n_root_searches;      /* of n_ll_searches: the searches that planned a root (diagnostic) */
  uint64_t schedule_digest;     /* as mrp_hl_solution.schedule_digest */
} mrp_hl_ta_solution;

/* One engine context on `device`, created and destroyed by the call.  stats (may be NULL): wall_seconds, rounds, ll_searches,
 * ll_expansions, solved, root_solved (instances solved at their first root).  n_instances == 0 succeeds. */
int mrp_hl_solve_cbs_ta_batch(int32_t device, const mrp_hl_ta_options* opt, int32_t n_instances,
                              const mrp_hl_ta_instance* instances, mrp_hl_ta_solution* solutions, mrp_hl_batch_stats* stats);

/* ---- ECBS with task assignment (ecbs_ta.hpp:94-352 over the Environment of example/ecbs_ta.cpp), batched ------------------
 * The reference as example/ecbs_ta.cpp compiles it: REBUILT_FOCAL_LIST and STYLE_MINROOT, Cost = int, low level AStarEpsilon
 * (MRP_LL_ASTAR_EPS_TA) under the same weight w.  Instances, options, solutions, tasks, the tie order among assignments of
 * equal cost, the limits and the error statuses are CBS-TA's above.  What differs:
 *   - A root plans its agents in index order, each against the paths of the agents before it only; a node's cost is the sum of
 *     its paths' costs, its LB the sum of their fmin, its focalHeuristic the number of all conflicts (mrp_ll_conflict's count).
 *   - The FIRST root is planned even when the first assignment is empty — every agent is then without a task and
 *     num_task_assignments stays 0 (ecbs_ta.hpp:104,117-137; CBS-TA gives up there).
 *   - The open list is ordered by cost alone; the focal list is rebuilt before every expansion from the open list's ordered
 *     walk, up to the first node with (float)cost > nextRootNodeCost, and is ordered by focalHeuristic, then cost.
 *     nextRootNodeCost is an int: LB * w, multiplied in binary32 and truncated, of the first root and then of the open
 *     list's top after every new-root attempt.
 *   - AFTER the two children of an expanded node are pushed, open.top().cost > nextRootNodeCost asks for the next assignment;
 *     a non-empty one is planned as a new root, which takes `id` and is pushed only when every agent got a path.
 * The reference reads three things it may not have; here they are defined:
 *   - an empty open list at the new-root test (ecbs_ta.hpp:302) counts as "ask for a new root";
 *   - an open list that is still empty after the attempt (:344) ends the instance MRP_HL_NO_SOLUTION;
 *   - an empty focal list at an expansion (:238; the truncation can leave the top's cost above nextRootNodeCost) ends the
 *     instance MRP_HL_LL_ERROR.
 * Round-based over all instances; a round makes at most one mrp_ll_assign_series_next, one mrp_ll_ta_eps_root_batch for the
 * new roots of at most 64 agents plus one mrp_ll_ta_eps_root_batch_w for the others (at most two root calls), and one
 * mrp_ll_search_batch of MRP_LL_ASTAR_EPS_TA jobs: for every expanded node its two child searches with the
 * node's paths as the shipped focal context.  With options.use_root_kernel = 0 a root is n_agents dependent jobs of that
 * batch instead, one agent per round, each with the paths before it as its context, and the driver scans and counts
 * itself; the results are the same.  One expansion can take several rounds either way (children, then assignment and root).
 * A NULL options pointer means use_root_kernel = 0, as do the Python and CLI front-ends: roots as jobs measured faster at
 * the reference shape with thousands of instances, the root call at a few hundred.
 * Environment, read once per call: MRP_HL_TA_DEVICE_PATHS=1 (off by default; same results, same stats but the times) keeps
 * every path in the engine's device-resident path store — the root call becomes mrp_ll_ta_eps_root_batch_stored, every job
 * carries MRP_LL_JOB_STORE_RESULT while a slot is free — and a job whose node has every other agent's path there names its
 * context by slot (mrp_ll_job.path_ids) instead of shipping it.  MRP_HL_TA_PATH_SLOTS=N: slots of that store (unset: four per
 * agent of the batch, between 256 and 65536; not tuned).  Instances of more than 64 agents ignore the knob — their contexts
 * ship and their roots go through the unstored call: a by-slot table of 256 agents does not fit a workgroup's path area.
 * w >= 1 (else MRP_LL_E_INVALID).  root_conflicts counts the expanded nodes with a conflict that carry the root flag (a
 * child is a copy of its parent, flag included). */
int mrp_hl_solve_ecbs_ta_batch(int32_t device, float w, const mrp_hl_ta_options* opt, int32_t n_instances,
                               const mrp_hl_ta_instance* instances, mrp_hl_ta_solution* solutions, mrp_hl_batch_stats* stats);

/* BASELINE.json configs[0] — `./a_star` on a text map (example/a_star.cpp:72-125,190-191) — is host plumbing: a single
 * 2-D A* (AStar::search a_star.hpp:63-161, neighbours Up, Down, Left, Right, unit costs, Manhattan heuristic), run on
 * the CPU with the reference's heap tie-breaks.  obstacle_mask[y * dimx + x] != 0 = '#'.  Returns the number of states
 * of the path (written to states_xy [cap][2] up to cap), 0 = "Planning NOT successful!", -1 = bad argument. */
int32_t mrp_hl_astar_grid2d(int32_t dimx, int32_t dimy, const uint8_t* obstacle_mask, int32_t start_x, int32_t start_y,
                            int32_t goal_x, int32_t goal_y, int32_t* states_xy, int32_t cap, int32_t* cost,
                            int64_t* expanded);

/* Seeded synthetic "32x32_obst204-shaped" instance: obstacles uniform without replacement, agents with
 * distinct starts and distinct goals, every goal in the start's 4-connected free component. splitmix64(seed).
 * Buffers: obstacles_xy [n_obstacles][2], starts_xy / goals_xy [n_agents][2]. Returns 0, or -1 if impossible. */
int mrp_hl_generate_instance(uint64_t seed, int32_t dimx, int32_t dimy, int32_t n_obstacles, int32_t n_agents,
                             int32_t* obstacles_xy, int32_t* starts_xy, int32_t* goals_xy);
/* The same for seeds seed0 .. seed0 + n - 1 in one call (host threads): instance k fills obstacles_xy[k][n_obstacles][2],
 * starts_xy[k][n_agents][2], goals_xy[k][n_agents][2].  Returns 0, or -1 if any instance was impossible. */
int mrp_hl_generate_instances(uint64_t seed0, int32_t n, int32_t dimx, int32_t dimy, int32_t n_obstacles,
                              int32_t n_agents, int32_t* obstacles_xy, int32_t* starts_xy, int32_t* goals_xy);

#ifdef __cplusplus
}
#endif
#endif /* MRP_HL_H */
