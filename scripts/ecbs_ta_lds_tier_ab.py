"""MRP_LL_ASTAR_EPS_TA, LDS tier against arena tier: the searches of the synthetic corpus (tests/ecbs_ta_corpus.py) that finish
in the LDS tier — the emulator says which (tests/eps_ta_tier_emu.py) —, `--copies` times over, as ONE batch, flagged
(MRP_LL_JOB_TRY_LDS) and unflagged, alternating in one process, `--runs` runs each after a warm-up of both.
usage: python scripts/ecbs_ta_lds_tier_ab.py [--copies 16] [--runs 3]
Prints one JSON line per run — wall and kernel seconds, expansions/s, and the device's own clock per expansion: prof[0] /
prof[1] (100 MHz ticks inside the LDS tier's search function / its expansions) for the flagged run, prof[2] / prof[3]
(the same for runJobTaEps, its staging included) for the unflagged one — and a summary line with the medians."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ecbs_ta_checker as checker  # noqa: E402
import ecbs_ta_corpus  # noqa: E402
import eps_ta_tier_emu as emu  # noqa: E402
from libmultirobotplanning_amd import ll  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--copies", type=int, default=16)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

with open(os.path.join(ROOT, "tests", "golden", "bench_instances.json")) as f:
    corpus, _ = ecbs_ta_corpus.generate(checker, json.load(f))
subset = [c for c in corpus if emu.in_tier(emu.run_case(c))]
expansions = sum(c["oracle"]["expanded"] for c in subset) * args.copies

eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=256)
try:
    maps, heurs = {}, {}

    def jobs_of(try_lds):
        jobs = []
        for c in subset:
            m, g = c["map"], c["goal"]
            key = id(m)
            if key not in maps:
                maps[key] = eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
            hid = -1
            if g is not None:
                if (key, tuple(g)) not in heurs:
                    heurs[(key, tuple(g))] = eng.upload_heuristic(maps[key], ecbs_ta_corpus.bfs_table(m["dimx"], m["dimy"], m["obstacles"], g))
                hid = heurs[(key, tuple(g))]
            jobs.append(ll.LLJob(map_id=maps[key], algo=ll.ASTAR_EPS_TA, start=c["start"], goal=g, agent_idx=c["agent"], w=c["w"],
                                 vertex_constraints=c["vc"], edge_constraints=c["ec"], ctx_paths=c["ctx"], max_expansions=c["cap"],
                                 heuristic_id=hid, try_lds=try_lds))
        return jobs * args.copies

    batches = {"lds": jobs_of(True), "arena": jobs_of(False)}
    for name in batches:  # warm-up of both
        eng.search_batch(batches[name])
    rows = {"lds": [], "arena": []}
    for run in range(args.runs):
        for name in ("lds", "arena"):
            eng.reset_stats()
            t0 = time.perf_counter()
            res = eng.search_batch(batches[name])
            wall = time.perf_counter() - t0
            st = eng.stats()
            assert sum(r.expanded for r in res) == expansions
            assert all(r.tier == (0 if name == "lds" else 1) for r in res)
            ticks, exp = (st["prof"][0], st["prof"][1]) if name == "lds" else (st["prof"][2], st["prof"][3])
            row = dict(path=name, run=run, searches=len(res), expansions=expansions, wall_s=round(wall, 5),
                       kernel_s=round(st["kernel_ms"] * 1e-3, 5), exp_per_s_wall=round(expansions / wall),
                       exp_per_s_kernel=round(expansions / (st["kernel_ms"] * 1e-3)) if st["kernel_ms"] > 0 else None,
                       search_ticks=ticks, search_expansions=exp, us_per_expansion_in_search=round(ticks / 100.0 / max(exp, 1), 4))
            rows[name].append(row)
            print(json.dumps(row), flush=True)
finally:
    eng.close()


def med(name, key):
    v = sorted(r[key] for r in rows[name])
    return v[len(v) // 2]


print(json.dumps(dict(summary=True, searches=len(subset) * args.copies, distinct_searches=len(subset), expansions=expansions, runs=args.runs,
                      lds_us_per_expansion=med("lds", "us_per_expansion_in_search"), arena_us_per_expansion=med("arena", "us_per_expansion_in_search"),
                      lds_exp_per_s_kernel=med("lds", "exp_per_s_kernel"), arena_exp_per_s_kernel=med("arena", "exp_per_s_kernel"),
                      lds_exp_per_s_wall=med("lds", "exp_per_s_wall"), arena_exp_per_s_wall=med("arena", "exp_per_s_wall"))))
