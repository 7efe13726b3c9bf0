"""What the runtime grants the front / heavy pair and what a solve call then runs (one JSON line): mrp_ll_session_tiers_geometry
before and after mrp_ll_session_front_tables, mrp_ll_session_occupancy, and — over one solve of 65 536 ten-agent instances
through hl.BatchSolver at sixteen threads — the engines, the front and heavy workgroups that ran a job, heavy_fallbacks.
Works on a build without the call too (it then reports the first geometry alone).  usage: front_tables_residency.py LABEL;
the driver's switch is MRP_HL_FRONT_TABLES / MRP_HL_SESSION_WGS in the environment (scripts/front_tables_ab.py sets them)."""
import json, os, sys
from libmultirobotplanning_amd import hl, ll
out = {"probe": "residency", "leg": sys.argv[1], "MRP_HL_FRONT_TABLES": os.environ.get("MRP_HL_FRONT_TABLES"),
       "MRP_HL_SESSION_WGS": os.environ.get("MRP_HL_SESSION_WGS")}
eng = ll.LowLevelEngine(device=0)
try:
    import ctypes
    def geo():
        occ, fr, hv = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        eng._lib.mrp_ll_session_tiers_geometry(eng._h, ctypes.byref(occ), ctypes.byref(fr), ctypes.byref(hv))
        return [occ.value, fr.value, hv.value]
    eng.configure_tiers(2048, 64, 2048)  # what the driver configures at ten agents
    out["tiers_geometry_before_call"] = geo()
    out["session_occupancy_eps"] = eng.session_occupancy(ll.ASTAR_EPS)
    if hasattr(eng, "session_front_tables"):
        eng.session_front_tables(True)
        out["tiers_geometry_after_call"] = geo()
        out["session_occupancy_eps_after_call"] = eng.session_occupancy(ll.ASTAR_EPS)
finally:
    eng.close()
s = hl.BatchSolver(device=0, n_threads=16)
try:
    ia = hl.generate_instances(5000000, 65536, 32, 32, 204, 10)
    prep = s.prepare(ia, want_paths=False)
    s.ll_stats(reset=True)
    _, st = s.solve_prepared(prep, algo=hl.ECBS, w=1.3, max_ll_expansions=50000, raw=True)
    lls = s.ll_stats()
    n_eng = max(lls["launches"] // 2, 1)
    out.update(engines=n_eng, launches=lls["launches"], heavy_fallbacks=lls["heavy_fallbacks"],
               front_workgroups_that_ran=lls["session_active_wgs"], heavy_workgroups_that_ran=lls["heavy_active_wgs"],
               front_workgroups_that_ran_per_engine=lls["session_active_wgs"] / n_eng,
               heavy_workgroups_that_ran_per_engine=lls["heavy_active_wgs"] / n_eng,
               wall_seconds=st["wall_seconds"], ll_expansions=st["ll_expansions"])
finally:
    s.close()
print(json.dumps(out))
