"""The A/B of the select-address stores and of the search loop's straight-line top ("stores without
exec regions, one test for the loop's exits"): the parent commit's build against this one, every run a process of its own
under its own time limit, one at a time, the builds alternating; one raw line per run is appended to OUT
(profiles/r19_loop_stores_ab.jsonl).  Stops at the first run that fails or runs into its time limit.
usage: python scripts/loop_stores_ab.py PARENT_TREE OUT.jsonl [profile] [headline] [parity] [legs]
PARENT_TREE: a checkout of the parent commit with its libraries built (python -m libmultirobotplanning_amd._build), and for
`profile` the diagnostic libraries: both trees' _build.build_variant('ctprof', ['-DMRP_CT_PROF']) and this tree's
'ctprof_es' (-DMRP_CT_PROF -DMRP_CT_EXEC_STORES: the masked stores) and 'ctprof_pl' (-DMRP_CT_PROF -DMRP_CT_PLAIN_LOOP: the
loop top that tests the goal twice and the limits one by one) and 'ctprof_es_pl' (both: the parent's stores and loop top with
the goal branch behind the loop, what the two parts are measured against).
headline: the bench command BENCH_r04.json records (--steps 20 --warmup 5), four rounds."""
import json, os, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 3:
    sys.exit(__doc__)
OUT = os.path.abspath(sys.argv[2])
os.makedirs(os.path.dirname(OUT), exist_ok=True)
TREE = {"parent": os.path.abspath(sys.argv[1]), "this": R}
ROUNDS = 4
PROFILES = (("parent", "parent", "ctprof"), ("this", "this", "ctprof"), ("this_exec_stores", "this", "ctprof_es"),
            ("this_plain_loop", "this", "ctprof_pl"), ("this_exec_stores_plain_loop", "this", "ctprof_es_pl"))


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


what = sys.argv[3:] or ["profile", "headline", "parity", "legs"]
if "profile" in what:  # shader cycles per phase of the instance that reads the rows from memory: this tree's script, each library
    for leg, tree, variant in PROFILES:
        run("profile", leg, "this", "scripts/ct_phase_profile.py", ["10", "64", "64", "front"],
            {"MRP_LL_LIB": os.path.join(TREE[tree], "libmultirobotplanning_amd", "lib", "libmrp_ll_%s.so" % variant)}, text=True)
if "headline" in what:
    for r in range(1, ROUNDS + 1):
        for tree in ("parent", "this"):
            run("headline", tree, tree, "bench.py", ["--gpus", "1", "--steps", "20", "--warmup", "5"], rnd=r)
if "parity" in what:
    line = run("parity", "this_full", "this", "bench.py", ["--gpus", "1", "--full", "--legs", "none"], limit=600)
    print("parity_whole_first_batch", line.get("parity_whole_first_batch"), "capped_in_first_timed_step",
          line.get("capped_in_first_timed_step"), flush=True)
if "legs" in what:
    for leg in ("agents50", "agents100"):
        for tree in ("parent", "this"):
            line = run("legs", "%s_%s" % (leg, tree), tree, "bench.py", ["--gpus", "1", "--full", "--no-cpu-baseline", "--legs", leg], limit=400)
            w = (line.get("by_workload") or {}).get(leg) or {}
            print("          %s: %.5g expansions/s, %.5g instances/s, solved %s of %s" % (
                leg, w.get("value") or 0, w.get("instances_per_s") or 0, w.get("solved"), w.get("instances")), flush=True)
