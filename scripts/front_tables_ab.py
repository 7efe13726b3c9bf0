"""The A/B of mrp_ll_session_front_tables: the parent commit's build against this one, every run a
process of its own, one at a time, legs alternating; one raw line per run is appended to OUT (profiles/r09_front_tables_ab.jsonl).
Stops at the first run that fails or runs into its time limit.
usage: python scripts/front_tables_ab.py PARENT_TREE OUT.jsonl [residency] [gain] [cost] [heavy] [legs] [parity]
PARENT_TREE: a checkout of the parent commit with its libraries built (python -m libmultirobotplanning_amd._build)."""
import json, os, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 3:
    sys.exit(__doc__)
OUT = os.path.abspath(sys.argv[2])
os.makedirs(os.path.dirname(OUT), exist_ok=True)
TREE = {"parent": os.path.abspath(sys.argv[1]), "this": R}
PARENT_FRONT = 322  # the parent's plan per engine: (256 * 12 - 3 * 160) / 8 - 2


def run(section, leg, tree, script, args, env=None, limit=240, rnd=None):
    e = dict(os.environ)
    e.update(env or {})
    e["PYTHONPATH"] = TREE[tree]
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(TREE[tree], script) if script == "bench.py" else os.path.join(R, script)] + args,
                           cwd=TREE[tree], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired:
        print("TIME LIMIT", section, leg, flush=True)
        sys.exit(124)
    if p.returncode != 0:
        print("FAILED", section, leg, p.returncode, p.stderr.decode()[-1500:], flush=True)
        sys.exit(p.returncode if p.returncode > 0 else 1)
    line = json.loads(p.stdout.decode().strip().splitlines()[-1])
    rec = {"section": section, "leg": leg, "build": tree, "round": rnd, "args": " ".join(args), "env": env or {}, "result": line}
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")
    v = line.get("value")
    t = line.get("tiers") or {}
    print("%-10s %-22s r%s  %s  %.0f s  front %.3f us/exp busy %.3f heavy busy %.3f" % (
        section, leg, rnd, ("%.4g" % v) if v else "-", time.time() - t0, t.get("front_us_per_expansion", 0),
        t.get("front_workgroups_busy_fraction", 0), t.get("heavy_workgroups_busy_fraction", 0)), flush=True)
    return line


what = sys.argv[3:] or ["residency", "gain", "cost", "heavy", "legs"]
if "residency" in what:
    run("residency", "parent", "parent", "scripts/front_tables_residency.py", ["parent"])
    run("residency", "this_memory", "this", "scripts/front_tables_residency.py", ["this_memory"], {"MRP_HL_FRONT_TABLES": "memory"})
    run("residency", "this_lds", "this", "scripts/front_tables_residency.py", ["this_lds"], {"MRP_HL_FRONT_TABLES": "lds"})
    run("residency", "this_memory_parent_front_count", "this", "scripts/front_tables_residency.py", ["this_memory_322"],
        {"MRP_HL_FRONT_TABLES": "memory", "MRP_HL_SESSION_WGS": str(PARENT_FRONT)})
if "gain" in what:
    for r in (1, 2, 3):
        run("gain", "parent", "parent", "bench.py", ["--gpus", "1"], rnd=r)
        run("gain", "this", "this", "bench.py", ["--gpus", "1"], rnd=r)
if "cost" in what:
    for r in (1, 2, 3):
        run("cost", "parent", "parent", "bench.py", ["--gpus", "1"], rnd=r)
        run("cost", "this_memory_parent_front_count", "this", "bench.py", ["--gpus", "1"],
            {"MRP_HL_FRONT_TABLES": "memory", "MRP_HL_SESSION_WGS": str(PARENT_FRONT)}, rnd=r)
if "heavy" in what:
    for h in (160, 192, 224):
        run("heavy", "this_heavy%d" % h, "this", "bench.py", ["--gpus", "1", "--steps", "1", "--warmup", "1"], {"MRP_HL_HEAVY_WGS": str(h)})
if "legs" in what:
    for leg in ("agents50", "agents100"):
        for tree in ("parent", "this"):
            run("legs", "%s_%s" % (leg, tree), tree, "bench.py", ["--gpus", "1", "--full", "--no-cpu-baseline", "--legs", leg], limit=400)
        for mode in ("memory", "lds"):  # the switch set, whatever the default is at this agent count
            run("legs", "%s_this_%s" % (leg, mode), "this", "bench.py", ["--gpus", "1", "--full", "--no-cpu-baseline", "--legs", leg],
                {"MRP_HL_FRONT_TABLES": mode}, limit=400)
if "parity" in what:
    line = run("parity", "this_full", "this", "bench.py", ["--gpus", "1", "--full", "--legs", "none"], limit=600)
    print("parity_whole_first_batch", line.get("parity_whole_first_batch"), flush=True)
