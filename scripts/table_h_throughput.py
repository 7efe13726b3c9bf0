"""Shortest-path heuristic against Manhattan on the flagship shape: N synthetic 32x32_obst204-shaped ten-agent ECBS instances
at w = 1.3, once through mrp_hl_solve_batch with mode = 1 (Manhattan in rounds: the like-for-like baseline) and once through
mrp_hl_solve_batch_table_h.  For both: instances/s, the sum of expansions, us per expansion.  Then, on one engine, what the
drivers' statistics do not hold: the tables' computation on its own (one mrp_ll_compute_heuristics for every goal), and the
share of searches per tier for the instances' unconstrained root searches, plain and with MRP_LL_JOB_TABLE_H.
usage: python scripts/table_h_throughput.py [N=4096] [seed0=700000]   (prints one JSON line)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libmultirobotplanning_amd import hl, ll  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
SEED0 = int(sys.argv[2]) if len(sys.argv) > 2 else 700000
W, CAP = 1.3, 200000
arrays = hl.generate_instances(SEED0, N, 32, 32, 204, 10)
insts = [arrays[k] for k in range(N)]


def figures(res, st):
    exp = st["ll_expansions"]
    return dict(wall_s=round(st["wall_seconds"], 4), instances_per_s=round(N / st["wall_seconds"], 1), solved=int(st["solved"]),
                expansions=int(exp), searches=int(st["ll_searches"]), rounds=int(st["rounds"]),
                us_per_expansion=round(1e6 * st["wall_seconds"] / exp, 4) if exp else None,
                cost=int(sum(r["cost"] for r in res if r["status"] == hl.SOLVED)))


solver = hl.BatchSolver(device=0)
try:
    solver.solve(insts[:64], algo=hl.ECBS, w=W, max_ll_expansions=CAP, mode=1, want_paths=False)  # warm-up
    manhattan = figures(*solver.solve(insts, algo=hl.ECBS, w=W, max_ll_expansions=CAP, mode=1, want_paths=False))
finally:
    solver.close()
hl.solve_batch_table_h(insts[:64], algo=hl.ECBS, w=W, max_ll_expansions=CAP, want_paths=False)  # warm-up
table_h = figures(*hl.solve_batch_table_h(insts, algo=hl.ECBS, w=W, max_ll_expansions=CAP, want_paths=False))

eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=1024)
try:
    maps = [eng.upload_map(32, 32, i["obstacles"]) for i in insts]
    eng.sync_maps()
    pairs = [(maps[k], g) for k, i in enumerate(insts) for g in i["goals"]]
    t0 = time.perf_counter()
    hids = eng.compute_heuristics([p[0] for p in pairs], [p[1] for p in pairs])
    tables_s = time.perf_counter() - t0
    tiers = {}
    for name, flag in (("manhattan", False), ("table_h", True)):
        jobs, q = [], 0
        for k, i in enumerate(insts):
            for a in range(len(i["starts"])):
                jobs.append(ll.LLJob(map_id=maps[k], algo=ll.ASTAR_EPS, start=i["starts"][a], goal=i["goals"][a], agent_idx=a, w=W,
                                     max_expansions=CAP, table_h=flag, heuristic_id=hids[q] if flag else 0))
                q += 1
        share = {}
        for lo in range(0, len(jobs), 8192):
            for r in eng.search_batch(jobs[lo:lo + 8192], states_cap=1):
                share[r.tier] = share.get(r.tier, 0) + 1
        tiers[name] = {str(t): round(n / len(jobs), 4) for t, n in sorted(share.items())}
finally:
    eng.close()
print(json.dumps(dict(instances=N, seed0=SEED0, w=W, manhattan_rounds=manhattan, table_h=table_h,
                      tables=len(pairs), tables_compute_s=round(tables_s, 4), root_search_tier_share=tiers)))
