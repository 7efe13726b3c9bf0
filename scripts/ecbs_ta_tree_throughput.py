"""ECBS-TA on the device: instances per second of the batched driver (mrp_hl_solve_ecbs_ta_batch, the time of its rounds:
tables and the series' optima are set up before) with roots through mrp_ll_ta_eps_root_batch (use_root_kernel 1) and as
dependent MRP_LL_ASTAR_EPS_TA jobs (0), the answers compared.  Workload: generated 32 x 32 instances with 204 obstacles, ten
agents, twenty potential goals shared by all agents of an instance, w = 1.3.  The forms alternate, --repeats runs each
after one warm-up run each; reported: the median, every run, and the spread (max - min) / median.
--device-paths adds both forms once more under MRP_HL_TA_DEVICE_PATHS=1 (paths in the engine's path store, contexts by slot;
--path-slots sets MRP_HL_TA_PATH_SLOTS), interleaved with the other two, answers compared with theirs.
--agents N above 64: the instances come from the wide corpus generator (tests/ta_wide_corpus.py instance(seed, N, pool):
32 x 32, 100 obstacles, 1 - 3 potential goals per agent among the six nearest of --pool cells, default min(256, 2 N)), seeds
0 .. instances - 1, every tree under --max-hl expansions (default 20: deterministic counters, bounded time); the root call is
then mrp_ll_ta_eps_root_batch_w.  E.g. --agents 96 --instances 16 and --agents 256 --instances 4.
usage: python scripts/ecbs_ta_tree_throughput.py [--instances 2048] [--w 1.3] [--device-paths]  (prints one JSON line)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libmultirobotplanning_amd import hl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=2048)
ap.add_argument("--agents", type=int, default=10)
ap.add_argument("--goals", type=int, default=20)
ap.add_argument("--maps", type=int, default=16)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--w", type=float, default=1.3)
ap.add_argument("--device-paths", action="store_true")
ap.add_argument("--path-slots", type=int, default=0)
ap.add_argument("--pool", type=int, default=0)
ap.add_argument("--max-hl", type=int, default=-1)
args = ap.parse_args()
CAP = 128  # states per result buffer


def component(dim, obst):
    """The largest connected set of free cells."""
    free = {(x, y) for y in range(dim) for x in range(dim)} - obst
    best = []
    while free:
        todo = [free.pop()]
        comp = list(todo)
        while todo:
            x, y = todo.pop()
            for c in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                if c in free:
                    free.remove(c)
                    todo.append(c)
                    comp.append(c)
        best = comp if len(comp) > len(best) else best
    return sorted(best)


def median(v):
    return sorted(v)[len(v) // 2]


rng = np.random.default_rng(3)
worlds = []
WIDE = args.agents > 64
MAX_HL = args.max_hl if args.max_hl >= 0 or not WIDE else 20
if WIDE:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ta_wide_corpus  # noqa: E402
    pool = args.pool or min(256, 2 * args.agents)
    insts = [ta_wide_corpus.instance(seed, args.agents, pool) for seed in range(args.instances)]
for _ in range(0 if WIDE else args.maps):
    cells = rng.permutation(32 * 32)[:204]
    obst = {(int(c) % 32, int(c) // 32) for c in cells}
    worlds.append((component(32, obst), [list(o) for o in sorted(obst)]))
insts = insts if WIDE else []
for k in range(0 if WIDE else args.instances):
    comp, obst = worlds[k % args.maps]
    pick = rng.permutation(len(comp))[:args.agents + args.goals]
    goals = [list(comp[i]) for i in pick[args.agents:]]
    insts.append(dict(dimx=32, dimy=32, obstacles=obst, starts=[list(comp[i]) for i in pick[:args.agents]],
                      potential_goals=[goals] * args.agents))
n = len(insts)

legs = [(1, False, "root_kernel"), (0, False, "root_jobs")]
if args.device_paths:
    legs += [(1, True, "root_kernel_device_paths"), (0, True, "root_jobs_device_paths")]
for knob in ("MRP_HL_TA_DEVICE_PATHS", "MRP_HL_TA_PATH_SLOTS"):
    os.environ.pop(knob, None)
walls, answers, last = {name: [] for _, _, name in legs}, {}, {}
for rep in range(args.repeats + 1):  # the first run of each form is the warm-up
    for use, paths, name in legs:
        if paths:  # (the driver reads its knobs once per call)
            os.environ["MRP_HL_TA_DEVICE_PATHS"] = "1"
            if args.path_slots:
                os.environ["MRP_HL_TA_PATH_SLOTS"] = str(args.path_slots)
        got, st = hl.solve_ecbs_ta_batch(insts, args.w, use_root_kernel=bool(use), max_hl_expansions=MAX_HL, path_cap=CAP)
        for knob in ("MRP_HL_TA_DEVICE_PATHS", "MRP_HL_TA_PATH_SLOTS"):
            os.environ.pop(knob, None)
        walls[name].append(st["wall_seconds"])
        last[name] = (got, st)
        answers[name] = [(g["status"], g["cost"], g["hl_expanded"], g["ll_expanded"], g["num_task_assignments"], g["digest"]) for g in got]
assert all(a == answers["root_kernel"] for a in answers.values())
result = dict(instances=n, agents=args.agents, potential_goals=args.goals, w=args.w, repeats=args.repeats, max_hl=MAX_HL,
              generator="ta_wide_corpus" if WIDE else "shared goals")
for _, _, name in legs:
    v = walls[name][1:]
    m = median(v)
    result[name] = dict(rounds_wall_s=round(m, 5), instances_per_s=round(n / m), walls=[round(x, 5) for x in v],
                        spread=round((max(v) - min(v)) / m, 4), rounds=last[name][1]["rounds"])
got, st = last["root_kernel"]
searches = sum(g["n_ll_searches"] for g in got)
result["breakdown"] = dict(solved=sum(1 for g in got if g["status"] == hl.SOLVED), searches=searches,
                           root_search_share=round(sum(g["n_root_searches"] for g in got) / max(searches, 1), 4),
                           solved_at_first_root_share=round(st["root_solved"] / n, 4), hl_expanded=sum(g["hl_expanded"] for g in got),
                           task_assignments=sum(g["num_task_assignments"] for g in got))
result["speedup_root_kernel_over_jobs"] = round(result["root_jobs"]["rounds_wall_s"] / result["root_kernel"]["rounds_wall_s"], 3)
print(json.dumps(result))
