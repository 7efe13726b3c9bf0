"""Shortest-path heuristic tables: the host's path against the device's, on the same machine in the same run.

  (a) what a C caller did before mrp_ll_compute_heuristics existed: a queue BFS per goal on the host, mrp_ll_upload_heuristic
      per table, one mrp_ll_sync_maps (scripts/micro/heur_host_path.cpp, g++ -O2, one core);
  (b) mrp_ll_compute_heuristics for the same (map, goal) pairs: one call, one launch.

Shapes: 1 024 / 16 384 / 65 536 tables over sixteen shipped 32 x 32 maps, and 64 tables on a 255 x 255 map with 20 % random
obstacles.  Per shape: one warm-up of each leg, then `--reps` repetitions with the legs alternating; every leg starts from
mrp_ll_release_maps + the map uploads (the device buffer keeps its capacity, so no repetition pays an allocation) and
ends with the tables usable by a search (leg (a): after the sync; leg (b): the call returns after the kernel).  Times
are host wall clock around calls that end in a device synchronise.  Leg (b)'s tables are compared with leg (a)'s through
mrp_ll_read_heuristic before anything is reported.

usage: python scripts/heuristic_tables.py [--reps 7] [--out profiles/heuristic_tables.json]   (needs the MI355X)"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libmultirobotplanning_amd import ll  # noqa: E402

I32P = ctypes.POINTER(ctypes.c_int32)


def host_path_lib():
    build = os.path.join(ROOT, "scripts", "micro", "bin")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, "libheur_host_path.so")
    src = os.path.join(ROOT, "scripts", "micro", "heur_host_path.cpp")
    libdir = os.path.join(ROOT, "libmultirobotplanning_amd", "lib")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", out,
                               src, "-L", libdir, "-lmrp_ll", "-Wl,-rpath,$ORIGIN/../../../libmultirobotplanning_amd/lib"])
    L = ctypes.CDLL(out)
    L.heur_host_path.restype = ctypes.c_int
    L.heur_host_path.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, I32P,
                                 ctypes.c_int32, I32P, I32P, ctypes.POINTER(ctypes.c_double)]
    return L


def free_cells(dimx, dimy, obstacles):
    blocked = np.zeros((dimy, dimx), dtype=bool)
    for x, y in obstacles:
        blocked[y, x] = True
    ys, xs = np.nonzero(~blocked)
    return np.stack([xs, ys], axis=1).astype(np.int32)


def shapes():
    with open(os.path.join(ROOT, "tests", "golden", "bench_instances.json")) as f:
        bench = json.load(f)
    names = sorted(k for k in bench if k.startswith("map_32by32_"))[:16]
    maps32 = [dict(dimx=32, dimy=32, obstacles=np.asarray(bench[k]["obstacles"], dtype=np.int32).reshape(-1, 2)) for k in names]
    rng = np.random.default_rng(255)
    mask = rng.random((255, 255)) < 0.2
    ys, xs = np.nonzero(mask)
    big = dict(dimx=255, dimy=255, obstacles=np.stack([xs, ys], axis=1).astype(np.int32))
    out = []
    for n in (1024, 16384, 65536):
        per = n // len(maps32)
        goals = []
        for k, m in enumerate(maps32):
            fc = free_cells(32, 32, m["obstacles"])
            goals.append(fc[np.random.default_rng(k).integers(0, len(fc), per)])
        out.append(("%d tables, 16 shipped 32x32 maps" % n, maps32, goals))
    fc = free_cells(255, 255, big["obstacles"])
    out.append(("64 tables, 255x255 map, 20% obstacles", [big], [fc[rng.integers(0, len(fc), 64)]]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heuristic_tables.json"))
    args = ap.parse_args()
    H = host_path_lib()
    eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=64, max_cells=65025)
    lib, h = eng._lib, eng._h

    def upload_maps(maps):
        eng.release_maps()
        return [eng.upload_map(m["dimx"], m["dimy"], m["obstacles"]) for m in maps]

    def leg_a(maps, goals):
        mids = upload_maps(maps)
        eng.sync_maps()
        ids, split = [], np.zeros(3)
        t0 = time.perf_counter()
        for mid, m, g in zip(mids, maps, goals):
            g = np.ascontiguousarray(g)
            out = np.zeros(len(g), dtype=np.int32)
            ms = (ctypes.c_double * 3)()
            rc = H.heur_host_path(h, mid, m["dimx"], m["dimy"], len(m["obstacles"]),
                                  np.ascontiguousarray(m["obstacles"]).ctypes.data_as(I32P), len(g), g.ctypes.data_as(I32P),
                                  out.ctypes.data_as(I32P), ms)
            assert rc == 0, rc
            split += np.asarray(list(ms))
            ids.append(out)
        return (time.perf_counter() - t0) * 1e3, np.concatenate(ids), split

    def leg_b(maps, goals):
        mids = upload_maps(maps)
        eng.sync_maps()
        mid_arr = np.ascontiguousarray(np.concatenate([np.full(len(g), mid, dtype=np.int32) for mid, g in zip(mids, goals)]))
        g_arr = np.ascontiguousarray(np.concatenate(goals).astype(np.int32))
        out = np.zeros(len(mid_arr), dtype=np.int32)
        k0 = eng.stats()["kernel_ms"]
        t0 = time.perf_counter()
        rc = lib.mrp_ll_compute_heuristics(h, len(mid_arr), mid_arr.ctypes.data_as(I32P), g_arr.ctypes.data_as(I32P),
                                           out.ctypes.data_as(I32P))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return ms, out, eng.stats()["kernel_ms"] - k0

    def read(hid, m):
        dist = np.zeros((m["dimy"], m["dimx"]), dtype=np.int32)
        assert lib.mrp_ll_read_heuristic(h, int(hid), dist.ctypes.data_as(I32P)) == 0
        return dist

    results = []
    try:
        for name, maps, goals in shapes():
            n = sum(len(g) for g in goals)
            # warm-up of both legs, and the check: the device's tables equal the host's
            _, ids_a, _ = leg_a(maps, goals)
            sample = sorted(set(np.linspace(0, n - 1, 24).astype(int).tolist()))
            owner = np.concatenate([np.full(len(g), i) for i, g in enumerate(goals)])  # table -> index of its map
            want = [read(ids_a[k], maps[owner[k]]) for k in sample]
            assert all(w.min() == 0 and (w < 2 ** 31 - 1).sum() > 1 for w in want)
            _, ids_b, _ = leg_b(maps, goals)
            for k, w in zip(sample, want):
                assert np.array_equal(read(ids_b[k], maps[owner[k]]), w), (name, k)
            a, b, kern, split = [], [], [], np.zeros(3)
            for _ in range(args.reps):
                ms, _, sp = leg_a(maps, goals)
                a.append(ms)
                split += sp / args.reps
                ms, _, km = leg_b(maps, goals)
                b.append(ms)
                kern.append(km)
            ma, mb = statistics.median(a), statistics.median(b)
            results.append(dict(shape=name, tables=n, reps=args.reps,
                                host_bfs_upload_sync_ms=dict(median=round(ma, 3), min=round(min(a), 3), max=round(max(a), 3),
                                                             mean_bfs=round(split[0], 3), mean_upload=round(split[1], 3),
                                                             mean_sync=round(split[2], 3)),
                                compute_heuristics_ms=dict(median=round(mb, 3), min=round(min(b), 3), max=round(max(b), 3),
                                                           median_kernel=round(statistics.median(kern), 3)),
                                ratio_host_over_device=round(ma / mb, 2)))
            print(json.dumps(results[-1]), flush=True)
    finally:
        eng.close()
    doc = dict(tool="scripts/heuristic_tables.py", version=ll.load_library().mrp_ll_version().decode(),
               note="wall-clock ms per leg; leg (a) is one host core (g++ -O2 queue BFS + mrp_ll_upload_heuristic + "
                    "mrp_ll_sync_maps), leg (b) one mrp_ll_compute_heuristics call; legs alternate, one warm-up each",
               results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
