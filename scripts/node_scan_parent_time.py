"""Device time of a child's conflict scan from what its parent's scan established (mrp_ll_submit_node) against the full scan
(mrp_ll_submit_scan): whole-job ticks (mrp_ll_stats.prof[4], 100 MHz) of the jobs of scripts/node_scan_time.py — one child
job per agent of the shipped agents10 / 20 / 50 / 100 ex0 inputs — unflagged, with MRP_LL_JOB_SCAN_CONFLICTS, and with
MRP_LL_JOB_SCAN_FROM_PARENT at clean_before = the parent's first-conflict time and = 0, as a batch and inside an A*-epsilon
session, alternating, median of five.  The bases come from the engine's own scan of the parent node.
Usage: python scripts/node_scan_parent_time.py [OUT.json]  (needs the GPU)"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from libmultirobotplanning_amd import ll
import test_node_scan_gpu as T

with open(os.path.join(ROOT, "tests", "golden", "bench_instances.json")) as f:
    corpus = json.load(f)
out = []
eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=512)
try:
    eng.path_store_reserve(4096)
    slot0 = 0
    for n in (10, 20, 50, 100):
        name = "map_32by32_obst204_agents%d_ex0" % n
        if name not in corpus:
            print("missing", name)
            continue
        node = T.Node(eng, corpus[name], slot0=slot0)
        slot0 += 2 * n
        parent = eng.conflict_scan([node.paths])[0]
        longest = max(len(p) for p in node.paths)
        first = parent["time"] if parent["found"] == 1 else longest - 1
        ids = [node.slot0 + b for b in range(n)]

        def jobs(kind):
            if kind == "plain":
                return node.jobs(scan=False)
            if kind == "full":
                return node.jobs(scan=True)
            return node.jobs(scan=True, path_ids=ids, scan_base=(parent["count"], first if kind == "parent_first" else 0))

        kinds = ("plain", "full", "parent_first", "parent_zero")
        for mode in ("batch", "session"):
            if mode == "session":
                eng.session_begin_algo(ll.ASTAR_EPS, 0)
            try:
                want = eng.search_batch_scan(jobs("full"))  # warm; and the answer every flagged form has to give
                ticks = {k: [] for k in kinds}
                fallback = 0
                for rep in range(5):
                    for kind in kinds:
                        eng.reset_stats()
                        res, conf = eng.search_batch_scan(jobs(kind))
                        assert all(r.status == ll.OK for r in res)
                        assert kind == "plain" or conf == want[1], kind
                        ticks[kind].append(eng.stats()["prof"][4] / len(res))
                        others = [max(len(p) for b, p in enumerate(node.paths) if b != a) for a in range(n)]
                        fallback = sum(max(others[a], res[a].n_states) != max(others[a], len(node.paths[a])) for a in range(n))
            finally:
                if mode == "session":
                    eng.session_end()
            med = {k: sorted(v)[len(v) // 2] / 100.0 for k, v in ticks.items()}
            row = dict(agents=n, mode=mode, longest_path=longest, jobs=n, parent_count=parent["count"], parent_first_time=first,
                       jobs_with_another_horizon=fallback, job_us=med,
                       scan_us_per_child={k: med[k] - med["plain"] for k in kinds if k != "plain"},
                       all_us={k: [t / 100.0 for t in v] for k, v in ticks.items()})
            print(json.dumps(row), flush=True)
            out.append(row)
finally:
    eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
