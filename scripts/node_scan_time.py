"""Device time of the conflict scan behind a child's search (mrp_ll_submit_scan): whole-job ticks (mrp_ll_stats.prof[4],
100 MHz) of flagged against unflagged jobs, one child job per agent of the shipped agents10 / 20 / 50 / 100 ex0 inputs (every
agent planned alone, then again under one vertex constraint with the others named by path-store slot), as a batch and inside an
A*-epsilon session, alternating, median of five.  Usage: python scripts/node_scan_time.py [OUT.json]  (needs the GPU)"""
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
        inst = corpus[name]
        node = T.Node(eng, inst, slot0=slot0)
        slot0 += 2 * n
        longest = max(len(p) for p in node.paths)
        for mode in ("batch", "session"):
            if mode == "session":
                eng.session_begin_algo(ll.ASTAR_EPS, 0)
            try:
                eng.search_batch_scan(node.jobs(scan=True))  # warm
                ticks = {True: [], False: []}
                exp = 0
                for rep in range(5):
                    for scan in (False, True):
                        eng.reset_stats()
                        res, conf = eng.search_batch_scan(node.jobs(scan=scan))
                        assert all(r.status == ll.OK for r in res)
                        exp = sum(r.expanded for r in res)
                        ticks[scan].append(eng.stats()["prof"][4] / len(res))
            finally:
                if mode == "session":
                    eng.session_end()
            med = {k: sorted(v)[len(v) // 2] for k, v in ticks.items()}
            row = dict(agents=n, mode=mode, longest_path=longest, jobs=n, expansions_per_job=exp / n,
                       job_us_unflagged=med[False] / 100.0, job_us_flagged=med[True] / 100.0,
                       scan_us_per_child=(med[True] - med[False]) / 100.0,
                       all_us_unflagged=[t / 100.0 for t in ticks[False]], all_us_flagged=[t / 100.0 for t in ticks[True]])
            print(json.dumps(row), flush=True)
            out.append(row)
finally:
    eng.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
