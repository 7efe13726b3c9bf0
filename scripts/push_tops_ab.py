"""The A/B of the expansion's push step and of the heap roots kept in a register ("pushes per lane, roots
kept"): the parent commit's build against this one, every run a process of its own under its own time limit, one at a time,
the builds alternating; one raw line per run is appended to OUT (profiles/r15_push_tops_ab.jsonl).  Stops at the first run
that fails or runs into its time limit.
usage: python scripts/push_tops_ab.py PARENT_TREE OUT.jsonl [profile] [headline] [parity] [legs50]
PARENT_TREE: a checkout of the parent commit with its libraries built (python -m libmultirobotplanning_amd._build), and for
`profile` the diagnostic libraries: both trees' _build.build_variant('ctprof', ['-DMRP_CT_PROF']) and this tree's
'ctprof_sp' (-DMRP_CT_PROF -DMRP_CT_SCALAR_PUSHES: the push step off), 'ctprof_kt' (-DMRP_CT_PROF -DMRP_CT_KEEP_TOPS: the kept
roots on as well) and 'ctprof_kt_sp' (-DMRP_CT_PROF -DMRP_CT_KEEP_TOPS -DMRP_CT_SCALAR_PUSHES: the kept roots alone).
(The agents100 leg with MRP_HL_FRONT_TABLES=memory is left out on purpose: DESIGN.md section 7.)"""
import json, os, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 3:
    sys.exit(__doc__)
OUT = os.path.abspath(sys.argv[2])
os.makedirs(os.path.dirname(OUT), exist_ok=True)
TREE = {"parent": os.path.abspath(sys.argv[1]), "this": R}
ROUNDS = 4
PROFILES = (("parent", "parent", "ctprof"), ("this", "this", "ctprof"), ("this_scalar_pushes", "this", "ctprof_sp"),
            ("this_keep_tops", "this", "ctprof_kt"), ("this_keep_tops_scalar_pushes", "this", "ctprof_kt_sp"))


def run(section, leg, tree, script, args, env=None, limit=240, rnd=None, text=False):
    e = dict(os.environ)
    e.update(env or {})
    e["PYTHONPATH"] = TREE[tree]
    t0 = time.time()
    path = os.path.join(TREE[tree], script) if script == "bench.py" else os.path.join(R, script)
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, path] + args, cwd=TREE[tree], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        print("FAILED" if p.returncode not in (124, 137) else "TIME LIMIT", section, leg, p.returncode, p.stderr.decode()[-1500:], flush=True)
        sys.exit(p.returncode if p.returncode > 0 else 1)
    out = p.stdout.decode().strip()
    line = {"text": out.splitlines()} if text else json.loads(out.splitlines()[-1])
    rec = {"section": section, "leg": leg, "build": tree, "round": rnd, "args": " ".join(args), "env": env or {}, "result": line}
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")
    if text:
        print("%-9s %-24s %.0f s\n%s" % (section, leg, time.time() - t0, out), flush=True)
        return line
    t = line.get("tiers") or {}
    print("%-9s %-24s r%s  %.5g  %.0f s  front %.4f us/exp (beyond %.4f) busy %.3f heavy busy %.3f handed over %s capped %s" % (
        section, leg, rnd, line.get("value") or 0, time.time() - t0, t.get("front_us_per_expansion", 0),
        t.get("beyond_front_us_per_expansion", 0), t.get("front_workgroups_busy_fraction", 0),
        t.get("heavy_workgroups_busy_fraction", 0), t.get("searches_handed_over"), line.get("capped_in_first_timed_step")), flush=True)
    return line


what = sys.argv[3:] or ["profile", "headline", "parity", "legs50"]
if "profile" in what:  # shader cycles per phase of the instance that reads the rows from memory: this tree's script, each library
    for leg, tree, variant in PROFILES:
        run("profile", leg, "this", "scripts/ct_phase_profile.py", ["10", "64", "64", "front"],
            {"MRP_LL_LIB": os.path.join(TREE[tree], "libmultirobotplanning_amd", "lib", "libmrp_ll_%s.so" % variant)}, text=True)
if "headline" in what:
    for r in range(1, ROUNDS + 1):
        for tree in ("parent", "this"):
            run("headline", tree, tree, "bench.py", ["--gpus", "1", "--steps", "3", "--warmup", "1"], rnd=r)
if "parity" in what:
    line = run("parity", "this_full", "this", "bench.py", ["--gpus", "1", "--full", "--legs", "none"], limit=600)
    print("parity_whole_first_batch", line.get("parity_whole_first_batch"), "capped_in_first_timed_step",
          line.get("capped_in_first_timed_step"), flush=True)
if "legs50" in what:
    for tree in ("parent", "this"):
        line = run("legs", "agents50_%s" % tree, tree, "bench.py", ["--gpus", "1", "--full", "--no-cpu-baseline", "--legs", "agents50"], limit=400)
        w = (line.get("by_workload") or {}).get("agents50") or {}
        print("          agents50: %.5g expansions/s, %.5g instances/s, solved %s of %s" % (
            w.get("value") or 0, w.get("instances_per_s") or 0, w.get("solved"), w.get("instances")), flush=True)
