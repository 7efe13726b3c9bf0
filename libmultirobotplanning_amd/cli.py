"""Command-line front-ends with the reference's flags, input formats and output schemas.

    python -m libmultirobotplanning_amd.cli ecbs -i in.yaml -o out.yaml -w 1.3     (example/ecbs.cpp:524-623)
    python -m libmultirobotplanning_amd.cli cbs  -i in.yaml -o out.yaml            (example/cbs.cpp:571-667)
        ecbs / cbs: --heuristic shortest_path runs every low-level search with the true grid distance to its goal (the code
        example/cbs.cpp:445-557 carries switched off) instead of the default, manhattan; same output schema
    python -m libmultirobotplanning_amd.cli cbs_ta -i in.yaml -o out.yaml [--maxTaskAssignments N]   (example/cbs_ta.cpp:523-617:
        agents[].{name,start,potentialGoals}; statistics also has numTaskAssignments, and a state's t is its cost so far)
    python -m libmultirobotplanning_amd.cli ecbs_ta -i in.yaml -o out.yaml -w 1.3 [--maxTaskAssignments N]
                                                                                   (example/ecbs_ta.cpp:587-695, as cbs_ta)
        cbs_ta / ecbs_ta: at most 256 agents and 256 distinct potential goals; beyond that "Planning NOT successful!"
    python -m libmultirobotplanning_amd.cli sipp -i in.yaml -o out.yaml            (example/sipp.cpp:149-236)
    python -m libmultirobotplanning_amd.cli mapf_prioritized_sipp -i in.yaml -o out.yaml
                                                                                   (example/mapf_prioritized_sipp.cpp:157-295)
    python -m libmultirobotplanning_amd.cli a_star --startX 0 --startY 0 --goalX 2 --goalY 1 -m map.txt -o out.yaml
                                                                                   (example/a_star.cpp:128-213)
    python -m libmultirobotplanning_amd.cli shortest_path_heuristic -i in.yaml     (example/shortest_path_heuristic.cpp:40-156)
    python -m libmultirobotplanning_amd.cli assignment -i costs.txt -o out.yaml [--wide]    (example/assignment.cpp:11-86)
    python -m libmultirobotplanning_amd.cli next_best_assignment -i costs.txt -o out.yaml [--wide]
                                                                                   (example/next_best_assignment.cpp:11-92)

ecbs / cbs   input  (ecbs.cpp:554-574): map.dimensions [x, y], map.obstacles [[x, y]..], agents[].{name,start,goal}
             output (ecbs.cpp:584-617): statistics.{cost, makespan, runtime, highLevelExpanded, lowLevelExpanded} and
                                        schedule.agent<k>: [{x, y, t}..] — what example/visualize.py:63,103 consumes.
sipp         input  (sipp.cpp:181-205): start, goal, environment.{size, obstacles, collisionIntervals[].{location,intervals}}
             output (sipp.cpp:225-232): schedule.agent1: [{x, y, t}..]
mapf_prioritized_sipp  input as ecbs; output (mapf_prioritized_sipp.cpp:211-272): schedule.agent<k> ("[]" for an agent
             that could not be planned), then statistics.cost
a_star       text map, '#' = obstacle (a_star.cpp:163-178: width = longest line, height = lines incl. the empty one after
             the last newline, minus 1); output schedule.agent1 with t = index (a_star.cpp:207-213).  Host plumbing
             (BASELINE.json configs[0]): no GPU involved.
shortest_path_heuristic  input: map.dimensions, map.obstacles (agents are not read); prints what the reference's example
             prints, ShortestPathHeuristic::getValue((0, 0), (3, 0)) (shortest_path_heuristic.cpp:152-153; INT_MAX when
             there is no path) — the table of the goal cell is computed on the device (mrp_ll_compute_heuristics) and the
             one entry looked up there.  -o is accepted and, as in the reference (whose CSV dump is compiled out), unused.
assignment / next_best_assignment  input: text, one "agent -> task : cost" per line (assignment.cpp:41; a line that does
             not match is reported on stderr and skipped); agents and tasks are numbered in order of first appearance.
             output: "cost: C" and "assignment:" with "  agent: task" lines (assignment.cpp:78-83), resp. "solutions:"
             with one "  - cost: / assignment:" block per matching of the optimum's cardinality in non-decreasing order
             of cost, "  []" when there is none (next_best_assignment.cpp:73-89); agents in sorted name order, as
             std::map prints them.  Solved on the device (mrp_ll_assign_batch, mrp_ll_assign_series_*): at most 64
             agents, 64 tasks and costs up to 16 777 215; beyond that the tool says so and exits non-zero.  --wide takes
             the wide solver (mrp_ll_assign_batch_w, mrp_ll_assign_series_create_w): at most 256 of each.  The order among
             solutions of equal cost is the engine's (include/mrp_ll.h), not Boost's.
On failure the reference prints "Planning NOT successful!" (and, for ecbs / cbs, writes nothing); so does this tool.
Several input files may be given to ecbs / cbs / mapf_prioritized_sipp (-i a.yaml -i b.yaml ... with matching -o): they
are solved as one GPU batch.  Inputs are read with the package's own YAML-subset reader (yaml_subset.py): no PyYAML.
"""
import argparse
import re
import sys
from typing import Dict, List

from . import yaml_subset


def read_instance(path: str) -> Dict:
    cfg = yaml_subset.load(path)
    dim = cfg["map"]["dimensions"]
    return dict(dimx=int(dim[0]), dimy=int(dim[1]),
                obstacles=[[int(o[0]), int(o[1])] for o in (cfg["map"].get("obstacles") or [])],
                starts=[[int(a["start"][0]), int(a["start"][1])] for a in cfg["agents"]],
                goals=[[int(a["goal"][0]), int(a["goal"][1])] for a in cfg["agents"]])


def read_sipp(path: str) -> Dict:
    cfg = yaml_subset.load(path)
    env = cfg["environment"]
    ci = []
    for node in env.get("collisionIntervals") or []:
        for iv in node["intervals"]:
            ci.append([int(node["location"][0]), int(node["location"][1]), int(iv[0]), int(iv[1])])
    return dict(dimx=int(env["size"][0]), dimy=int(env["size"][1]),
                obstacles=[[int(o[0]), int(o[1])] for o in (env.get("obstacles") or [])],
                start=[int(v) for v in cfg["start"]], goal=[int(v) for v in cfg["goal"]], collision_intervals=ci)


def read_text_map(path: str):
    """a_star.cpp:163-178: std::getline until !good() — the empty read after the final newline counts as a line."""
    with open(path) as f:
        text = f.read()
    lines = text.split("\n")
    dimx = max(len(l) for l in lines)
    dimy = len(lines) - 1
    mask = [[1 if (x < len(lines[y]) and lines[y][x] == "#") else 0 for x in range(dimx)] for y in range(dimy)]
    return dimx, dimy, mask


def write_schedule(path: str, res: Dict, runtime: float) -> None:
    # written by hand to keep the reference's key order (ecbs.cpp:593-617)
    with open(path, "w") as out:
        out.write("statistics:\n")
        out.write("  cost: %d\n" % res["cost"])
        out.write("  makespan: %d\n" % res["makespan"])
        out.write("  runtime: %g\n" % runtime)
        out.write("  highLevelExpanded: %d\n" % res["hl_expanded"])
        out.write("  lowLevelExpanded: %d\n" % res["ll_expanded"])
        out.write("schedule:\n")
        for a, p in enumerate(res["paths"]):
            out.write("  agent%d:\n" % a)
            for t, (x, y) in enumerate(p):
                out.write("    - x: %d\n      y: %d\n      t: %d\n" % (x, y, t))


def read_ta_instance(path: str) -> Dict:
    """example/cbs_ta.cpp:543-566: map, agents[].start, agents[].potentialGoals."""
    cfg = yaml_subset.load(path)
    dim = cfg["map"]["dimensions"]
    return dict(dimx=int(dim[0]), dimy=int(dim[1]),
                obstacles=[[int(o[0]), int(o[1])] for o in (cfg["map"].get("obstacles") or [])],
                starts=[[int(a["start"][0]), int(a["start"][1])] for a in cfg["agents"]],
                potential_goals=[[[int(g[0]), int(g[1])] for g in (a.get("potentialGoals") or [])] for a in cfg["agents"]])


def main_cbs_ta(args, ap) -> int:
    """cbs_ta -i in.yaml -o out.yaml [--maxTaskAssignments N]: the output of example/cbs_ta.cpp:589-614.
    ecbs_ta -i in.yaml -o out.yaml -w W [--maxTaskAssignments N]: the output of example/ecbs_ta.cpp:655-689, which has the
    same form.  Both take at most 256 agents and 256 distinct potential goals."""
    from . import hl
    if len(args.input) != len(args.output):
        ap.error("give one -o per -i")
    insts = [read_ta_instance(p) for p in args.input]
    if args.algo == "ecbs_ta":
        res, st = hl.solve_ecbs_ta_batch(insts, args.suboptimality, max_task_assignments=args.maxTaskAssignments, device=args.device,
                                         max_ll_expansions=args.max_ll_expansions, path_cap=1024)
    else:
        res, st = hl.solve_cbs_ta_batch(insts, max_task_assignments=args.maxTaskAssignments, device=args.device,
                                        max_ll_expansions=args.max_ll_expansions, path_cap=1024)
    rc = 0
    for r, path in zip(res, args.output):
        if r["status"] != hl.SOLVED:
            print("Planning NOT successful!" + (" (harness cap)" if r["status"] == hl.CAP else ""))
            rc = 1 if r["status"] != hl.NO_SOLUTION else rc
            continue
        print("Planning successful! ")
        with open(path, "w") as out:
            out.write("statistics:\n")
            out.write("  cost: %d\n" % r["cost"])
            out.write("  makespan: %d\n" % r["makespan"])
            out.write("  runtime: %g\n" % st["wall_seconds"])
            out.write("  highLevelExpanded: %d\n" % r["hl_expanded"])
            out.write("  lowLevelExpanded: %d\n" % r["ll_expanded"])
            out.write("  numTaskAssignments: %d\n" % r["num_task_assignments"])
            out.write("schedule:\n")
            for a, p in enumerate(r["paths"]):
                out.write("  agent%d:\n" % a)
                _write_states(out, p)  # t: the state's cost so far, as the reference writes it (:606-610)
    return rc


def _write_states(out, states_xyt) -> None:
    for x, y, t in states_xyt:
        out.write("    - x: %d\n      y: %d\n      t: %d\n" % (x, y, t))


def main_mapf(args, ap) -> int:
    from . import hl
    if len(args.input) != len(args.output):
        ap.error("give one -o per -i")
    insts = [read_instance(p) for p in args.input]
    if args.heuristic == "shortest_path":  # the low level's h is the true grid distance to the goal (hl.solve_batch_table_h)
        res, st = hl.solve_batch_table_h(insts, algo=hl.ECBS if args.algo == "ecbs" else hl.CBS, w=args.suboptimality,
                                         max_ll_expansions=args.max_ll_expansions, n_threads=min(len(insts), 16),
                                         device=args.device, path_cap=1024)
    else:
        solver = hl.BatchSolver(device=args.device, n_threads=min(len(insts), 16))
        try:
            res, st = solver.solve(insts, algo=hl.ECBS if args.algo == "ecbs" else hl.CBS, w=args.suboptimality,
                                   max_ll_expansions=args.max_ll_expansions, path_cap=1024)
        finally:
            solver.close()
    rc = 0
    for r, out in zip(res, args.output):
        if r["status"] == hl.SOLVED:
            print("Planning successful! ")
            write_schedule(out, r, st["wall_seconds"])
        else:
            print("Planning NOT successful!" + (" (harness cap)" if r["status"] == hl.CAP else ""))
            rc = 1 if r["status"] != hl.NO_SOLUTION else rc
    return rc


def main_prioritized_sipp(args, ap) -> int:
    from . import hl
    if len(args.input) != len(args.output):
        ap.error("give one -o per -i")
    insts = [read_instance(p) for p in args.input]
    solver = hl.BatchSolver(device=args.device, n_threads=min(len(insts), 16), max_horizon=1024,
                            max_cells=max(4096, max(i["dimx"] * i["dimy"] for i in insts)))
    try:
        res, _ = solver.prioritized_sipp(insts, state_cap=2048)
    finally:
        solver.close()
    for r, path in zip(res, args.output):
        with open(path, "w") as out:  # mapf_prioritized_sipp.cpp:211-272
            out.write("schedule:\n")
            for a, sched in enumerate(r["schedules"]):
                print("Planning for agent %d" % a)
                out.write("  agent%d:\n" % a)
                if r["planned"][a]:
                    print("Planning successful! Total cost: %d" % (sched[-1][2]))
                    _write_states(out, sched)
                else:
                    print("Planning NOT successful!")
                    out.write("    []\n")
            out.write("statistics:\n  cost: %d\n" % r["cost"])
    return 0


def main_sipp(args, ap) -> int:
    from . import ll
    if len(args.input) != 1 or len(args.output) != 1:
        ap.error("sipp takes one -i and one -o")
    cfg = read_sipp(args.input[0])
    eng = ll.LowLevelEngine(device=args.device, n_tickets=1, slots=16, max_horizon=1024,
                            max_cells=max(4096, cfg["dimx"] * cfg["dimy"]))
    try:
        mid = eng.upload_map(cfg["dimx"], cfg["dimy"], cfg["obstacles"])
        r = eng.search_batch([ll.LLJob(map_id=mid, algo=ll.SIPP, start=cfg["start"], goal=cfg["goal"],
                                       collision_intervals=cfg["collision_intervals"])], states_cap=4096)[0]
    finally:
        eng.close()
    if not r.success:
        print("Planning NOT successful!")
        return 0
    print("Planning successful! Total cost: %d" % r.cost)  # sipp.cpp:213-223
    for k in range(len(r.actions)):
        t, x, y = r.states[k]
        print("%d: (%d,%d)->%s(cost: %d)" % (t, x, y, ll.ACTION_NAMES[r.actions[k]], r.action_costs[k]))
    t, x, y = r.states[-1]
    print("%d: (%d,%d)" % (t, x, y))
    with open(args.output[0], "w") as out:
        out.write("schedule:\n  agent1:\n")
        _write_states(out, [(x, y, t) for t, x, y in r.states])
    return 0


def main_a_star(args, ap) -> int:
    from . import hl
    for k in ("startX", "startY", "goalX", "goalY", "map"):
        if getattr(args, k) is None:
            ap.error("a_star needs --startX --startY --goalX --goalY -m -o")
    if len(args.output) != 1:
        ap.error("a_star takes one -o")
    dimx, dimy, mask = read_text_map(args.map)
    print("%d %d" % (dimx, dimy + 1))  # the reference prints the line count, not the height it passes on (a_star.cpp:179)
    states, cost, _ = ([], 0, 0) if dimx <= 0 or dimy <= 0 else hl.astar_grid2d(
        dimx, dimy, mask, [args.startX, args.startY], [args.goalX, args.goalY])
    with open(args.output[0], "w") as out:  # the file is created either way (a_star.cpp:194)
        if states:
            print("Planning successful! Total cost: %d" % cost)
            out.write("schedule:\n  agent1:\n")
            _write_states(out, [(x, y, t) for t, (x, y) in enumerate(states)])
        else:
            print("Planning NOT successful!")
    return 0


def main_shortest_path_heuristic(args, ap) -> int:
    from . import ll
    if len(args.input) != 1:
        ap.error("shortest_path_heuristic takes one -i")
    cfg = yaml_subset.load(args.input[0])
    dim = cfg["map"]["dimensions"]
    dimx, dimy = int(dim[0]), int(dim[1])
    if dimx < 4 or dimy < 1:
        ap.error("shortest_path_heuristic asks for getValue((0, 0), (3, 0)): the map must be at least 4 cells wide")
    obstacles = [[int(o[0]), int(o[1])] for o in (cfg["map"].get("obstacles") or [])]
    eng = ll.LowLevelEngine(device=args.device, n_tickets=1, slots=16, max_cells=max(4096, dimx * dimy))
    try:
        mid = eng.upload_map(dimx, dimy, obstacles)
        hid = eng.compute_heuristics([mid], [[3, 0]])[0]
        print(int(eng.heuristic_lookup([hid], [[0, 0]])[0]))
    finally:
        eng.close()
    return 0


_PAIR = re.compile(r"(\w+)\s*->\s*(\w+)\s*:\s*(\d+)")  # assignment.cpp:41


def read_assignment(path: str, limit: int = 64):
    """agent names, task names (order of first appearance) and the cost matrix with None where no line set a cost.
    limit: how many agents and tasks the solver takes (64; 256 with --wide)."""
    agents, tasks, cost = [], [], {}
    with open(path) as f:
        for line in f.read().splitlines():
            m = _PAIR.search(line)
            if not m:
                sys.stderr.write("Couldn't match line \"%s\"!\n" % line)
                continue
            a, t, c = m.group(1), m.group(2), int(m.group(3))
            if a not in agents:
                agents.append(a)
            if t not in tasks:
                tasks.append(t)
            key = (agents.index(a), tasks.index(t))
            cost[key] = min(c, cost.get(key, c))  # a pair given twice: two parallel edges, the cheaper one is used
    if len(agents) > limit or len(tasks) > limit:
        raise ValueError("%d agents and %d tasks: the device solver takes at most %d of each%s"
                         % (len(agents), len(tasks), limit, "" if limit > 64 else " (--wide: 256)"))
    if any(c > 16777215 for c in cost.values()):
        raise ValueError("a cost above 16777215 (2^24 - 1): the device solver does not take it")
    matrix = [[cost.get((a, t)) for t in range(len(tasks))] for a in range(len(agents))]
    return agents, tasks, matrix


def _pairs(agents, tasks, task_of):
    return sorted((agents[a], tasks[t]) for a, t in enumerate(task_of) if t >= 0)


def main_assignment(args, ap) -> int:
    from . import ll
    if len(args.input) != 1 or len(args.output) != 1:
        ap.error("%s takes one -i and one -o" % args.algo)
    try:
        agents, tasks, matrix = read_assignment(args.input[0], 256 if args.wide else 64)
    except ValueError as e:
        sys.stderr.write("%s: %s\n" % (args.algo, e))
        return 1
    prob = dict(cost=matrix, nA=len(agents), nT=len(tasks))
    eng = ll.LowLevelEngine(device=args.device, n_tickets=1, slots=16)
    try:
        with open(args.output[0], "w") as out:
            if args.algo == "assignment":
                r = eng.assign_batch([prob], wide=args.wide)[0]
                print("solution with cost: %d" % r.cost)
                out.write("cost: %d\nassignment:\n" % r.cost)
                for a, t in _pairs(agents, tasks, r.task_of):
                    print("%s: %s" % (a, t))
                    out.write("  %s: %s\n" % (a, t))
            else:
                series = eng.assign_series([prob], wide=args.wide)[0]
                out.write("solutions:\n")
                try:
                    count = 0
                    while True:
                        r = series.next()
                        if r.status != ll.OK or r.matched == 0:  # the empty solution ends the list
                            break
                        count += 1
                        out.write("  - cost: %d\n    assignment:\n" % r.cost)
                        for a, t in _pairs(agents, tasks, r.task_of):
                            out.write("      %s: %s\n" % (a, t))
                    if count == 0:
                        out.write("  []\n")
                finally:
                    series.close()
    finally:
        eng.close()
    return 0


def main(argv: List[str] = None) -> int:
    ap = argparse.ArgumentParser(prog="libmultirobotplanning_amd.cli")
    ap.add_argument("algo", choices=["ecbs", "cbs", "sipp", "mapf_prioritized_sipp", "a_star", "shortest_path_heuristic",
                                     "assignment", "next_best_assignment", "cbs_ta", "ecbs_ta"])
    ap.add_argument("-i", "--input", action="append", default=[], help="input file (YAML)")
    ap.add_argument("-o", "--output", action="append", default=[], help="output file (YAML)")
    ap.add_argument("-w", "--suboptimality", type=float, default=1.0, help="suboptimality bound (ecbs, ecbs_ta)")
    ap.add_argument("-m", "--map", help="input map (txt) (a_star)")
    for k in ("startX", "startY", "goalX", "goalY"):
        ap.add_argument("--" + k, type=int, help="a_star: %s" % k)
    ap.add_argument("--maxTaskAssignments", type=int, default=10 ** 9, help="cbs_ta, ecbs_ta: maximum number of task assignments to try")
    ap.add_argument("--wide", action="store_true",
                    help="assignment, next_best_assignment: the wide solver, at most 256 agents and 256 tasks (default: 64)")
    ap.add_argument("--heuristic", choices=["manhattan", "shortest_path"], default="manhattan",
                    help="ecbs, cbs: the low-level searches' admissible heuristic (shortest_path: the true grid distance to the goal, "
                         "from tables computed on the device)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-ll-expansions", type=int, default=-1, help="harness cap per instance (reference: none)")
    args = ap.parse_args(argv)
    if args.algo != "a_star" and not args.input:
        ap.error("-i is required")
    if args.algo == "shortest_path_heuristic":
        return main_shortest_path_heuristic(args, ap)
    if not args.output:
        ap.error("the following arguments are required: -o/--output")
    if args.algo in ("assignment", "next_best_assignment"):
        return main_assignment(args, ap)
    if args.algo in ("cbs_ta", "ecbs_ta"):
        return main_cbs_ta(args, ap)
    if args.algo in ("ecbs", "cbs"):
        return main_mapf(args, ap)
    if args.algo == "mapf_prioritized_sipp":
        return main_prioritized_sipp(args, ap)
    if args.algo == "sipp":
        return main_sipp(args, ap)
    return main_a_star(args, ap)


if __name__ == "__main__":
    sys.exit(main())
