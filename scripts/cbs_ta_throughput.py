"""CBS-TA on the device, two comparisons.  (1) Root nodes of CBS-TA conflict trees per second: mrp_ll_ta_root_batch against the same roots as n ordinary
MRP_LL_ASTAR_TA jobs of mrp_ll_search_batch plus mrp_ll_conflict_scan on their paths — kernels the root call does not
touch.  Workload: generated 32 x 32 instances, ten agents, twenty potential goals shared by all agents of an instance;
each root plans the instance's min-cost assignment (mrp_ll_assign_batch, gather form).  Wall clock of the C calls, marshalling
done once outside the timed region, median of --repeats after a warm-up; kernel time from stats.kernel_ms.
(2) Instances per second of the batched driver (mrp_hl_solve_cbs_ta_batch, the time of its rounds: tables and the series'
optima are set up before) on the same instances with use_root_kernel 1 and 0, same median, the answers compared; with the
share of searches that are root searches and the share of instances solved at their first root.
--agents N above 64: comparison (2) alone, on instances of the wide corpus generator (tests/ta_wide_corpus.py
instance(seed, N, pool): 32 x 32, 100 obstacles, 1 - 3 potential goals per agent among the six nearest of --pool cells, default
min(256, 2 N)), seeds 0 .. instances - 1, every tree under --max-hl expansions (default 20); the root call is then
mrp_ll_ta_root_batch_w.  E.g. --agents 96 --instances 16 and --agents 256 --instances 4.
usage: python scripts/cbs_ta_throughput.py [--instances 4096]  (prints one JSON line)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libmultirobotplanning_amd import ll  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=4096)
ap.add_argument("--agents", type=int, default=10)
ap.add_argument("--goals", type=int, default=20)
ap.add_argument("--maps", type=int, default=16)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--slots", type=int, default=1024)
ap.add_argument("--pool", type=int, default=0)
ap.add_argument("--max-hl", type=int, default=-1)
args = ap.parse_args()
WIDE = args.agents > 64
MAX_HL = args.max_hl if args.max_hl >= 0 or not WIDE else 20
CAP = 128  # states per result buffer (paths on these maps stay below it; a longer one would come back PATH_TRUNCATED)


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
eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=args.slots)
try:
    if WIDE:
        raise StopIteration  # (comparison (1) is the narrow root call's)
    # maps, and one table per (map, potential goal): one launch
    worlds = []
    for _ in range(args.maps):
        cells = rng.permutation(32 * 32)[:204]
        obst = {(int(c) % 32, int(c) // 32) for c in cells}
        worlds.append((eng.upload_map(32, 32, [list(o) for o in obst]), component(32, obst), [list(o) for o in sorted(obst)]))
    inst = []
    for k in range(args.instances):
        mid, comp, _ = worlds[k % args.maps]
        pick = rng.permutation(len(comp))[:args.agents + args.goals]
        inst.append((mid, [comp[i] for i in pick[:args.agents]], [comp[i] for i in pick[args.agents:]]))
    hids = eng.compute_heuristics([m for m, _, g in inst for _ in g], [list(c) for _, _, g in inst for c in g])
    hids = [hids[k * args.goals:(k + 1) * args.goals] for k in range(args.instances)]
    assign = eng.assign_batch([dict(n_agents=args.agents, n_tasks=args.goals, heuristic_ids=h, starts=s)
                               for (_, s, _), h in zip(inst, hids)])
    assert all(a.status == ll.OK and a.matched == args.agents for a in assign)
    roots = [ll.TaRoot(map_id=m, starts=s, goals=[g[t] for t in a.task_of], heuristic_ids=[h[t] for t in a.task_of])
             for (m, s, g), h, a in zip(inst, hids, assign)]
    n = len(roots)

    # ---- the root call
    croots, planned, conf, per_root, keep = eng._marshal_ta_roots(roots, CAP)
    walls, kernels = [], []
    for _ in range(args.repeats + 1):  # the first call is the warm-up (it also grows the staging)
        eng.reset_stats()
        t0 = time.perf_counter()
        rc = eng._lib.mrp_ll_ta_root_batch(eng._h, n, croots, planned.ctypes.data_as(ll.I32P), conf)
        walls.append(time.perf_counter() - t0)
        assert rc == 0, rc
        st = eng.stats()
        assert st["launches"] == 1
        kernels.append(st["kernel_ms"] * 1e-3)
    assert all(int(p) == args.agents for p in planned)
    root_call = dict(wall_s=round(median(walls[1:]), 5), kernel_s=round(median(kernels[1:]), 5), walls=[round(w, 5) for w in walls[1:]])
    found_root = [c.found for c in conf]
    count_root = [c.count for c in conf]
    searches = args.agents * n
    expansions = sum(int(per_root[i][1][a].expanded) for i in range(n) for a in range(args.agents))

    # ---- the same roots as ordinary jobs + the batch conflict scan
    jobs = [ll.LLJob(map_id=r.map_id, algo=ll.ASTAR_TA, start=s, goal=g, heuristic_id=h)
            for r in roots for s, g, h in zip(r.starts, r.goals, r.heuristic_ids)]
    cjobs, cres, bufs = eng._marshal(jobs, CAP)
    rc = eng._lib.mrp_ll_search_batch(eng._h, len(jobs), cjobs, cres)
    assert rc == 0, rc
    res = eng._results(len(jobs), CAP, cres, *bufs[1:])
    assert [int(per_root[i][1][a].expanded) for i in range(n) for a in range(args.agents)] == [r.expanded for r in res]
    lens = [r.n_states for r in res]
    set_first = np.arange(0, len(jobs) + 1, args.agents, dtype=np.int32)
    path_first = np.zeros(len(jobs) + 1, dtype=np.int32)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=path_first[1:])
    xy = np.ascontiguousarray(np.asarray([s[1:] for r in res for s in r.states], dtype=np.int32).reshape(-1, 2))
    out = (ll.mrp_ll_conflict * n)()
    walls, kernels, scans = [], [], []
    for _ in range(args.repeats + 1):
        eng.reset_stats()
        t0 = time.perf_counter()
        rc = eng._lib.mrp_ll_search_batch(eng._h, len(jobs), cjobs, cres)
        t1 = time.perf_counter()
        rc2 = eng._lib.mrp_ll_conflict_scan(eng._h, n, set_first.ctypes.data_as(ll.I32P), path_first.ctypes.data_as(ll.I32P),
                                            xy.ctypes.data_as(ll.I32P), out)
        t2 = time.perf_counter()
        assert rc == 0 and rc2 == 0, (rc, rc2)
        walls.append(t2 - t0)
        scans.append(t2 - t1)
        kernels.append(eng.stats()["kernel_ms"] * 1e-3)  # (the searches' launch; the scan's kernel is not in the statistics)
    assert [c.found for c in out] == found_root and [c.count for c in out] == count_root
    jobs_call = dict(wall_s=round(median(walls[1:]), 5), search_kernel_s=round(median(kernels[1:]), 5),
                     scan_wall_s=round(median(scans[1:]), 5), walls=[round(w, 5) for w in walls[1:]])
    result = dict(instances=n, agents=args.agents, potential_goals=args.goals, searches=searches, expansions=expansions,
                          roots_with_a_conflict=sum(1 for f in found_root if f == 1),
                          root_batch=dict(root_call, roots_per_s=round(n / root_call["wall_s"])),
                          jobs_plus_scan=dict(jobs_call, roots_per_s=round(n / jobs_call["wall_s"])),
                          speedup=round(jobs_call["wall_s"] / root_call["wall_s"], 3))
except StopIteration:
    n, result = args.instances, dict(instances=args.instances, agents=args.agents, generator="ta_wide_corpus", max_hl=MAX_HL)
finally:
    eng.close()

# ---- the driver, roots as one call against roots as ordinary jobs
from libmultirobotplanning_amd import hl  # noqa: E402

if WIDE:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ta_wide_corpus  # noqa: E402
    pool = args.pool or min(256, 2 * args.agents)
    dinst = [ta_wide_corpus.instance(seed, args.agents, pool) for seed in range(args.instances)]
dinst = dinst if WIDE else [dict(dimx=32, dimy=32, obstacles=worlds[k % args.maps][2], starts=[list(c) for c in s],
              potential_goals=[[list(c) for c in g]] * args.agents) for k, (_, s, g) in enumerate(inst)]
driver, answers = {}, {}
for use in (1, 0):
    walls, calls = [], []
    for _ in range(args.repeats + 1):
        t0 = time.perf_counter()
        got, st = hl.solve_cbs_ta_batch(dinst, use_root_kernel=bool(use), max_hl_expansions=MAX_HL, path_cap=CAP)
        calls.append(time.perf_counter() - t0)
        walls.append(st["wall_seconds"])
    answers[use] = [(g["status"], g["cost"], g["hl_expanded"], g["ll_expanded"], g["num_task_assignments"], g["digest"]) for g in got]
    w = median(walls[1:])
    driver[use] = dict(rounds_wall_s=round(w, 5), instances_per_s=round(n / w), walls=[round(x, 5) for x in walls[1:]],
                       whole_call_s=round(median(calls[1:]), 3), rounds=st["rounds"])
    if use == 1:
        searches_all = sum(g["n_ll_searches"] for g in got)
        result["driver_breakdown"] = dict(
            solved=sum(1 for g in got if g["status"] == hl.SOLVED), searches=searches_all,
            root_search_share=round(sum(g["n_root_searches"] for g in got) / searches_all, 4),
            solved_at_first_root_share=round(st["root_solved"] / n, 4),
            hl_expanded=sum(g["hl_expanded"] for g in got), task_assignments=sum(g["num_task_assignments"] for g in got))
assert answers[0] == answers[1]
result["driver_root_kernel"] = driver[1]
result["driver_root_jobs"] = driver[0]
result["driver_speedup"] = round(driver[0]["rounds_wall_s"] / driver[1]["rounds_wall_s"], 3)
print(json.dumps(result))
