"""Build recipe for the in-tree native libraries (hipcc, gfx950 only).

``libmrp_ll.so``  — HIP kernels + C-ABI of the low-level search engine (include/mrp_ll.h)
``libmrp_hl.so``  — host-side C++ conflict-tree drivers (CBS / ECBS) that call the C-ABI, instance generator, YAML I/O

Both are built into ``libmultirobotplanning_amd/lib/`` so they travel with the repo snapshot to the GPU box.
"""
import os
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_PKG, "csrc")
LIBDIR = os.path.join(_PKG, "lib")
INCLUDE = os.path.join(os.path.dirname(_PKG), "include")

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", INCLUDE]

TARGETS = {
    "libmrp_ll.so": dict(srcs=["ll_kernel.hip", "conflict_kernel.hip", "heur_kernel.hip", "assign_kernel.hip", "mrp_ll_host.cpp"],
                         deps=["ll_device.h", "ll_slot.h", "ll_compact.h", "ll_compact_ta_eps.h", "ll_arena_heap.h", "ll_arena_search.h", "ll_jobs.h", "ll_ta.h",
                               "ll_ta_root.h", "ll_sipp.h", "ll_node_scan.h", "wave_dev.h", "wave_dev_bool.h", "heur_bfs.h", "heur_layout.h",
                               "assign_wave.h", "assign_wave_wide.h", "assign_layout.h", "host/assign_pack.h", "host/assign_series.h",
                               "host/ll_assign_host.h", "host/ta_root_pack.h", "host/ll_ta_root_host.h", "host/ta_eps_root_pack.h",
                               "ll_launch.h", "host/ll_pack.h", "host/ll_sipp_table.h", "host/ll_unpack.h", "host/ll_ctx.h",
                               "host/ll_maps.h", "host/ll_heur_host.h", "host/ll_stores.h", "host/ll_batch.h",
                               "host/ll_session.h", "host/ll_session_jobs.h", "host/ll_submit.h", "../../include/mrp_ll.h"],
                         extra=[]),
    "libmrp_hl.so": dict(srcs=["hl/mrp_hl.cpp", "hl/mrp_hl_ta.cpp", "hl/mrp_hl_ecbs_ta.cpp"],
                         deps=["hl/exact_heap.hpp", "hl/ta_tree_base.hpp", "hl/cbs_ta_tree.hpp", "hl/ecbs_ta_tree.hpp", "hl/ta_batch_setup.hpp", "hl/ta_rounds.hpp", "hl/grid_mapf.hpp", "hl/ct_solver.hpp",
                                                       "hl/ct_session.hpp", "hl/grid2d_astar.hpp", "hl/instance_io.hpp",
                                                       "hl/solve_knobs.hpp", "hl/launch_plan.hpp", "hl/rounds_driver.hpp",
                                                       "hl/sipp_drivers.hpp", "hl/ct_stepped.hpp",
                                                       "../../include/mrp_ll.h", "../../include/mrp_hl.h"],
                         extra=["-pthread", "-L", LIBDIR, "-lmrp_ll", "-Wl,-rpath,$ORIGIN"]),
}


def _stale(out, paths):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.exists(p) and os.path.getmtime(p) > t for p in paths)


def build_trace(verbose=False):
    """Diagnostic variant of libmrp_ll.so (-DMRP_LL_TRACE): the kernel writes progress words to a host-mapped buffer
    that mrp_ll_wait dumps if a launch does not finish within 10 s (run with MRP_LL_DEBUG=1 MRP_LL_LIB=<this file>)."""
    os.makedirs(LIBDIR, exist_ok=True)
    spec = TARGETS["libmrp_ll.so"]
    out = os.path.join(LIBDIR, "libmrp_ll_trace.so")
    cmd = [HIPCC] + COMMON + ["-DMRP_LL_TRACE", "-o", out] + [os.path.join(CSRC, s) for s in spec["srcs"]]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return out


def build_variant(name, defines, verbose=False):
    """A/B build of libmrp_ll.so with extra -D flags (e.g. build_variant("fences", ["-DMRP_LL_SESSION_FENCES"]));
    use it under the host drivers with LD_PRELOAD=<returned path>."""
    os.makedirs(LIBDIR, exist_ok=True)
    spec = TARGETS["libmrp_ll.so"]
    out = os.path.join(LIBDIR, "libmrp_ll_%s.so" % name)
    cmd = [HIPCC] + COMMON + list(defines) + ["-o", out] + [os.path.join(CSRC, s) for s in spec["srcs"]]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return out


def build(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    built = []
    for name, spec in TARGETS.items():
        srcs = [os.path.join(CSRC, s) for s in spec["srcs"]]
        if not all(os.path.exists(s) for s in srcs):
            continue
        deps = srcs + [os.path.normpath(os.path.join(CSRC, d)) for d in spec["deps"]]
        out = os.path.join(LIBDIR, name)
        if force or _stale(out, deps):
            cmd = [HIPCC] + COMMON + spec["extra"] + ["-o", out] + srcs
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd, cwd=CSRC)
        built.append(out)
    return built


if __name__ == "__main__":
    import sys
    for p in build(force="--force" in sys.argv, verbose=True):
        print("built", p)
    if "--trace" in sys.argv:
        print("built", build_trace(verbose=True))
