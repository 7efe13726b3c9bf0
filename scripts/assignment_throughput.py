"""Assignment throughput: batches of random dense problems through mrp_ll_assign_batch (problems per second from
stats.kernel_ms and from the wall clock of the C call, marshalling done once outside the timed region) and one
mrp_ll_assign_series_next step over many live series.
usage: python scripts/assignment_throughput.py [--problems 65536] [--series 4096]  (prints one JSON line)
       python scripts/assignment_throughput.py --wide --dim N [--problems 4096]
           the same N x N problems through mrp_ll_assign_batch_w and, for N <= 64, through mrp_ll_assign_batch; the cost
           rows' source follows MRP_LL_ASSIGN_LDS_BYTES (unset: LDS rows while they fit 64 KiB; 0: memory rows)"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libmultirobotplanning_amd import ll  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--problems", type=int, default=65536)
ap.add_argument("--series", type=int, default=4096)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--wide", action="store_true", help="measure the wide call at --dim")
ap.add_argument("--dim", type=int, default=64)
args = ap.parse_args()


def batch_rate(eng, dim, n, rng, wide=False, cost=None):
    if cost is None:
        cost = rng.integers(0, 1000, size=(n, dim, dim), dtype=np.int32)
    carr, keep, dims = eng._marshal_assign([dict(cost=cost[k]) for k in range(n)], wide)
    call = eng._lib.mrp_ll_assign_batch_w if wide else eng._lib.mrp_ll_assign_batch
    cres, task_of = eng._assign_results(dims)
    walls, kernels = [], []
    for _ in range(args.repeats + 1):  # the first call is the warm-up (it also grows the staging)
        eng.reset_stats()
        t0 = time.perf_counter()
        rc = call(eng._h, n, carr, cres)
        walls.append(time.perf_counter() - t0)
        assert rc == 0, rc
        st = eng.stats()
        assert st["launches"] == 1
        kernels.append(st["kernel_ms"] * 1e-3)
    assert all(r.status == ll.OK and r.matched == dim for r in cres)
    wall, kern = sorted(walls[1:])[len(walls[1:]) // 2], sorted(kernels[1:])[len(kernels[1:]) // 2]
    return dict(dim=dim, problems=n, wide=wide, total_cost=int(sum(r.cost for r in cres)), kernel_s=round(kern, 5), problems_per_s_kernel=round(n / kern) if kern > 0 else None,
                wall_s=round(wall, 5), problems_per_s_wall=round(n / wall), walls=[round(w, 5) for w in walls[1:]])


def series_step(eng, dim, n, rng):
    cost = rng.integers(0, 1000, size=(n, dim, dim), dtype=np.int32)
    series = eng.assign_series([dict(cost=cost[k]) for k in range(n)])
    hs = (ctypes.c_void_p * n)(*[s._h for s in series])
    cres, task_of = eng._assign_results([dim] * n)
    walls, kernels = [], []
    for _ in range(args.repeats + 1):
        eng.reset_stats()
        t0 = time.perf_counter()
        rc = eng._lib.mrp_ll_assign_series_next(eng._h, n, hs, cres)
        walls.append(time.perf_counter() - t0)
        assert rc == 0, rc
        st = eng.stats()
        assert st["launches"] == 1 and all(r.status == ll.OK for r in cres)
        kernels.append(st["kernel_ms"] * 1e-3)
    for s in series:
        s.close()
    wall, kern = sorted(walls[1:])[len(walls[1:]) // 2], sorted(kernels[1:])[len(kernels[1:]) // 2]
    return dict(dim=dim, series=n, children_per_step_at_most=n * dim, step_kernel_s=round(kern, 5), step_wall_s=round(wall, 5),
                walls=[round(w, 5) for w in walls[1:]])


rng = np.random.default_rng(1)
eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=16)
try:
    if args.wide:
        n = min(args.problems, 4096) if args.problems == 65536 else args.problems
        cost = rng.integers(0, 1000, size=(n, args.dim, args.dim), dtype=np.int32)
        out = dict(lds_budget=os.environ.get("MRP_LL_ASSIGN_LDS_BYTES", "default"))
        if args.dim <= 64:
            out["narrow"] = batch_rate(eng, args.dim, n, rng, False, cost)
        out["wide"] = batch_rate(eng, args.dim, n, rng, True, cost)
        if "narrow" in out:
            assert out["narrow"]["total_cost"] == out["wide"]["total_cost"]
        print(json.dumps(out))
        sys.exit(0)
    out = dict(batch_10x10=batch_rate(eng, 10, args.problems, rng), batch_64x64=batch_rate(eng, 64, args.problems, rng),
               series_step_10x10=series_step(eng, 10, args.series, rng))
finally:
    eng.close()
print(json.dumps(out))
