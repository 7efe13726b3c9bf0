"""MRP_LL_ASTAR_EPS_TA throughput: the synthetic corpus of tests/ecbs_ta_corpus.py as ONE batch on the GPU, next to the CPU
checker's single-core rate on the same cases.  usage: python scripts/ecbs_ta_throughput.py  (prints one JSON line)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ecbs_ta_checker as checker  # noqa: E402
import ecbs_ta_corpus  # noqa: E402
from test_ecbs_ta_parity_gpu import _jobs  # noqa: E402
from libmultirobotplanning_amd import ll  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "bench_instances.json")) as f:
    corpus, _ = ecbs_ta_corpus.generate(checker, json.load(f))
expansions = sum(c["oracle"]["expanded"] for c in corpus)
t0 = time.perf_counter()
for c in corpus:  # the checker again, timed: marshalling included, one core
    checker.ll_search(c["map"], c["start"], c["goal"], c["vc"], c["ec"], w=c["w"], agent_idx=c["agent"], ctx_paths=c["ctx"],
                      cap_expansions=c["cap"])
cpu_s = time.perf_counter() - t0
eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=256)
try:
    jobs = _jobs(eng, corpus, ({}, {}))
    eng.search_batch(jobs)  # warm-up
    walls, kernels = [], []
    for _ in range(5):
        eng.reset_stats()
        t0 = time.perf_counter()
        res = eng.search_batch(jobs)
        walls.append(time.perf_counter() - t0)
        kernels.append(eng.stats()["kernel_ms"] * 1e-3)
    assert sum(r.expanded for r in res) == expansions
finally:
    eng.close()
wall, kern = sorted(walls)[2], sorted(kernels)[2]
print(json.dumps(dict(cases=len(corpus), expansions=expansions, largest_search=max(c["oracle"]["expanded"] for c in corpus),
                      cpu_checker_s=round(cpu_s, 4), cpu_checker_exp_per_s=round(expansions / cpu_s),
                      gpu_batch_wall_s=round(wall, 4), gpu_batch_exp_per_s=round(expansions / wall),
                      gpu_kernel_s=round(kern, 4), gpu_kernel_exp_per_s=round(expansions / kern) if kern > 0 else None,
                      walls=[round(x, 4) for x in walls])))
