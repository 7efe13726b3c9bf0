"""Cases, CPU model and ctypes marshalling of the root-chain tests (tests/test_root_chain_cases_cpu.py on the CPU,
tests/test_root_chain_gpu.py on the device): MRP_LL_JOB_ROOT_CHAIN of include/mrp_ll.h, the root step of an ECBS conflict
tree as one job.  HIP-free: the model needs the oracle alone, the marshalling helper the ctypes records of ll.py (the
library is never loaded here).

An instance is dict(dimx, dimy, obstacles, starts, goals).  A case is dict(name, inst, w, cls, parked, model): `model` is
chain_model(inst, w) — the whole chain, unlimited budget —, `cls` one of CLASSES for a generated case or "hand" for a
hand-made one, `parked` whether the root's first conflict is with an agent that stands on its goal behind the end of its path.

The model restates the header's contract:
  agent a = first .. end - 1 is planned by oracle.ll_search(ECBS, ..., ctx_paths = the paths of the agents before a, [] for the
  rest, w, cap_expansions = what the budget has left); the chain stops BEHIND the first agent without a path (expansion cap;
  the reference never returns "no solution" on these maps: a Wait is always possible); the agents behind are NOT_RUN with zeroed
  fields; the job's n_states = results filled in, expanded = their sum; cost / fmin = the conflict count and the encoded first
  conflict of oracle.conflict_scan when first == 0 and every agent of the instance got a path, else -1 / -1.
A record (of the model and of the engine, see Batch.result) is dict(status, cost, fmin, n_states, expanded, states, actions);
the model leaves cost and fmin None where the header calls them invalid (status != OK): same() skips them.

Classes of a complete root (classify): the oracle's scan says whether there is a conflict and at which time step t0; a
brute-force look at t0 lists the vertex pairs V and the edge pairs E there (and must agree with the oracle on the first one):
  free                            no conflict
  vertex                          V only
  edge                            E only
  both_same_t                     V and E, min(V) < min(E)  (lexicographic (i, j))
  both_same_t_edge_pair_smaller   V and E, min(E) < min(V): a scan that orders by pair before type reports the edge pair
  parked (a flag beside the class) the first conflict is a vertex conflict at t0 >= len(path) of one of its two agents
"""
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402

OK, NO_SOLUTION, CAP_EXPANSIONS, BAD_JOB, NOT_RUN = 0, 1, 2, 5, 8              # include/mrp_ll.h MRP_LL_*
JOB_STORE_RESULT, JOB_ROOT_CHAIN, JOB_HEAVY, JOB_SCAN_CONFLICTS = 1, 4, 8, 16  # mrp_ll_job.flags
ASTAR_EPS = 1

ORACLE_CAP = 3000  # expansion cap of every oracle search without a budget: an unreachable goal never ends otherwise
# Bounds of a selected search (test_root_chain_cases_cpu.py asserts them; ll_compact.h states the tier's limits):
MAX_STATES = 40      # states of a path
MAX_EXPANDED = 203   # an expansion pushes at most 5 nodes and the tier wants 5 free entries: 5 * 203 + 1 + 5 <= 1023
CLASSES = ("free", "vertex", "edge", "both_same_t", "both_same_t_edge_pair_smaller")

# (dimension, obstacles, agents, w, seeds): the generated shapes
SHAPES = (
    (5, 5, 6, 1.0, range(0, 250)),
    (6, 8, 5, 1.0, range(0, 250)),
    (8, 14, 6, 1.0, range(0, 250)),
    (8, 14, 8, 1.3, range(0, 250)),
    (8, 12, 10, 1.3, range(0, 250)),
)
PER_SHAPE_COMMON, PER_SHAPE_RARE = 1, 2  # cases per shape of free / vertex / edge, and of the two both_* classes and parked


class Unbounded(Exception):
    """An oracle search without a budget ran into ORACLE_CAP: the instance is not a case."""


def gen_instance(dim, n_obst, n_agents, seed):
    """dim x dim map with n_obst obstacle cells, n_agents distinct free start cells and n_agents distinct free goal cells."""
    rng = np.random.RandomState(1000003 * dim + 10007 * n_obst + 101 * n_agents + seed)
    cells = rng.permutation(dim * dim)
    free = cells[n_obst:]
    goals = rng.permutation(free)[:n_agents]
    xy = lambda c: [int(c % dim), int(c // dim)]  # noqa: E731
    return dict(dimx=dim, dimy=dim, obstacles=[xy(c) for c in cells[:n_obst]], starts=[xy(c) for c in free[:n_agents]],
                goals=[xy(c) for c in goals])


def encode_conflict(scan):
    """mrp_ll.h: time << 24 | type << 16 | agent1 << 8 | agent2, or -1."""
    if not scan["found"]:
        return -1
    return (scan["time"] << 24) | (scan["type"] << 16) | (scan["agent1"] << 8) | scan["agent2"]


def not_run():
    return dict(status=NOT_RUN, cost=0, fmin=0, n_states=0, expanded=0, states=[], actions=[])


def plan(inst, w, a, ctx_paths, left=-1, vc=()):
    """One oracle search of agent a as a record; `left` < 0: no budget (ORACLE_CAP as the safety cap -> Unbounded)."""
    o = oracle.ll_search(oracle.ECBS, inst, a, inst["starts"][a], inst["goals"][a], vertex_constraints=vc,
                         ctx_paths=ctx_paths, w=w, cap_expansions=left if left >= 0 else ORACLE_CAP)
    if o["rc"] == -1:
        if left < 0:
            raise Unbounded((a, o["expanded"]))
        return dict(status=CAP_EXPANSIONS, cost=None, fmin=None, n_states=0, expanded=o["expanded"], states=[], actions=[])
    assert o["success"], "the reference's search ends only with a path or at the cap"
    return dict(status=OK, cost=o["cost"], fmin=o["fmin"], n_states=len(o["states"]), expanded=o["expanded"],
                states=o["states"], actions=o["actions"])


def chain_model(inst, w, first=0, count=0, budget=-1, prior_paths=None, break_before=None):
    """The chain job (agent_idx = first, chain_count = count, max_expansions = budget) as the header promises it.
    prior_paths: the paths [[x, y], ...] of the agents 0 .. first - 1 (what their path-store slots hold).
    break_before(a, record): True = agent a's search "outgrows the LDS tier" (the chain ends in FRONT of it).
    Returns dict(results = records of the agents first .. n - 1, n_states, expanded, cost, fmin, paths = [[x, y], ...] per
    agent of the instance, None where there is none)."""
    n = len(inst["starts"])
    assert 0 <= first < n
    end = min(n, first + count) if count > 0 else n
    paths = [None] * n
    for a in range(first):
        paths[a] = [list(c) for c in prior_paths[a]]
    results, left, total, done, stopped = [], budget, 0, 0, False
    for a in range(first, n):
        if stopped or a >= end:
            results.append(not_run())
            continue
        r = plan(inst, w, a, [paths[b] if b < a else [] for b in range(n)], left)
        if break_before is not None and break_before(a, r):
            stopped = True
            results.append(not_run())
            continue
        results.append(r)
        done += 1
        total += r["expanded"]
        if r["status"] != OK:
            stopped = True
            continue
        paths[a] = [s[1:] for s in r["states"]]
        if left >= 0:
            left = max(left - r["expanded"], 0)
    cost = fmin = -1
    if first == 0 and end == n and done == n and not stopped:
        scan = oracle.conflict_scan(paths)
        cost, fmin = scan["count"], encode_conflict(scan)
    return dict(results=results, n_states=done, expanded=total, cost=cost, fmin=fmin, paths=paths)


def same(got, want):
    """The fields in which an engine record differs from a model record (None in the model: not compared)."""
    return [k for k in ("status", "cost", "fmin", "n_states", "expanded", "states", "actions")
            if want[k] is not None and got[k] != want[k]]


def state_at(path, t):
    return path[min(t, len(path) - 1)]


def conflicts_at(paths, t):
    """Brute force: the vertex pairs and the edge pairs (i, j), i < j, at time step t, each in lexicographic order."""
    V, E = [], []
    for i in range(len(paths)):
        for j in range(i + 1, len(paths)):
            if state_at(paths[i], t) == state_at(paths[j], t):
                V.append((i, j))
            if state_at(paths[i], t) == state_at(paths[j], t + 1) and state_at(paths[i], t + 1) == state_at(paths[j], t):
                E.append((i, j))
    return V, E


def classify(paths):
    """(class, parked) of a complete root."""
    scan = oracle.conflict_scan(paths)
    if not scan["found"]:
        return "free", False
    t0 = scan["time"]
    V, E = conflicts_at(paths, t0)
    first = (0,) + V[0] if V else (1,) + E[0]
    assert first == (scan["type"], scan["agent1"], scan["agent2"]), ("oracle scan vs brute force", scan, V, E)
    assert t0 < max(len(p) for p in paths) - 1 and all(conflicts_at(paths, t) == ([], []) for t in range(t0))
    parked = scan["type"] == 0 and (t0 >= len(paths[scan["agent1"]]) or t0 >= len(paths[scan["agent2"]]))
    if V and E:
        return ("both_same_t_edge_pair_smaller" if E[0] < V[0] else "both_same_t"), parked
    return ("vertex" if V else "edge"), parked


def in_tier(model):
    """Every search of the chain stays inside the bounds this module selects by."""
    return all(r["n_states"] <= MAX_STATES and r["expanded"] <= MAX_EXPANDED for r in model["results"])


def make_case(name, inst, w, cls=None):
    model = chain_model(inst, w)
    assert model["n_states"] == len(inst["starts"])
    c, parked = classify(model["paths"])
    return dict(name=name, inst=inst, w=w, cls=cls or c, parked=parked, model=model)


def first_complete(dim, n_obst, n_agents, w, seeds):
    """The first seed of the shape whose root is complete and inside the bounds (hand-made shapes)."""
    for seed in seeds:
        inst = gen_instance(dim, n_obst, n_agents, seed)
        try:
            model = chain_model(inst, w)
        except Unbounded:
            continue
        if in_tier(model):
            return seed, inst
    raise AssertionError("no complete root among the seeds", (dim, n_obst, n_agents))


def hand_cases():
    """The edges no generator is trusted with: one agent; every agent on its goal (no time step to scan: cost 0, fmin -1);
    16 and 17 agents (n_agents_pad 16 and 32: the two sides of the focal table's column step)."""
    out = [make_case("hand/n1", dict(dimx=5, dimy=5, obstacles=[[2, 2], [1, 3]], starts=[[0, 0]], goals=[[4, 3]]), 1.0, "hand")]
    spots = [[0, 0], [3, 1], [5, 5], [2, 4]]
    out.append(make_case("hand/all_on_goal", dict(dimx=6, dimy=6, obstacles=[[1, 1], [4, 2]], starts=spots, goals=spots), 1.3, "hand"))
    for n in (16, 17):
        seed, inst = first_complete(10, 8, n, 1.3, range(0, 50))
        out.append(make_case("hand/n%d_10x10_seed%d" % (n, seed), inst, 1.3, "hand"))
    return out


@functools.lru_cache(maxsize=None)
def survey():
    """Every seed of every shape: (counts per shape of the classes, "parked", "capped" = some search hit ORACLE_CAP, "big" = a
    complete root with a search outside the bounds; the selected cases).  Per shape the first PER_SHAPE_COMMON roots of free,
    vertex and edge and the first PER_SHAPE_RARE of both_same_t, both_same_t_edge_pair_smaller and of the parked ones."""
    counts, cases = [], []
    for dim, n_obst, n_agents, w, seeds in SHAPES:
        cnt = dict.fromkeys(CLASSES + ("parked", "capped", "big"), 0)
        taken = dict.fromkeys(CLASSES + ("parked",), 0)
        for seed in seeds:
            inst = gen_instance(dim, n_obst, n_agents, seed)
            try:
                model = chain_model(inst, w)
            except Unbounded:
                cnt["capped"] += 1
                continue
            if not in_tier(model):
                cnt["big"] += 1
                continue
            cls, parked = classify(model["paths"])
            cnt[cls] += 1
            cnt["parked"] += 1 if parked else 0
            quota = PER_SHAPE_COMMON if cls in ("free", "vertex", "edge") else PER_SHAPE_RARE
            want = taken[cls] < quota or (parked and taken["parked"] < PER_SHAPE_RARE)
            if want:
                taken[cls] += 1
                taken["parked"] += 1 if parked else 0
                cases.append(dict(name="%dx%d_o%d_a%d_w%.1f/seed%d" % (dim, dim, n_obst, n_agents, w, seed), inst=inst, w=w,
                                  cls=cls, parked=parked, model=model))
        counts.append(cnt)
    return counts, cases


@functools.lru_cache(maxsize=None)
def select_cases():
    """The chains of the tests: the survey's selection and the hand-made edges.  Computed once; nobody changes a case."""
    return tuple(survey()[1]) + tuple(hand_cases())


def break_case():
    """A root whose agent BREAK_K outgrows a tier of BREAK_ROWS time steps (mrp_ll_configure_tiers' lds_rows) while the agents
    in front of it cannot: a 16 x 3 map without obstacles at w = 1.0.  The narrow tier leaves at the pop of a node that is no
    goal at t > lds_rows - 2 (ll_jobs.h narrowMaxT, ll_compact.h compactSearch).  Agents 0 .. 2 walk at most 4 steps: at w = 1.0
    they expand nodes of f <= cost only, t <= 4 < BREAK_ROWS - 2.  Agent 3 walks 14 steps along the middle row: the nodes of
    its path at t = 11 .. 13 are no goals, are expanded by any search that finds it, and 11 > BREAK_ROWS - 2 = 10.
    Agent 4 parks on (11, 1) from t = 2 on, where agent 3 comes by at t = 11: the root's conflicts depend on agent 3's path."""
    inst = dict(dimx=16, dimy=3, obstacles=[],
                starts=[[0, 0], [5, 2], [9, 0], [0, 1], [13, 1], [15, 2]],
                goals=[[2, 0], [5, 0], [6, 0], [14, 1], [11, 1], [13, 2]])
    return inst, 1.0


BREAK_ROWS, BREAK_K = 12, 3


# ---- ctypes marshalling (include/mrp_ll.h through the records of libmultirobotplanning_amd/ll.py) ---------------------------

class Batch:
    """The jobs of one submit call.  add_chain / add_job return the job's index; build() makes the arrays; result(i) decodes."""

    def __init__(self, cap=64):
        from libmultirobotplanning_amd import ll
        self.ll, self.cap, self.specs, self.keep = ll, cap, [], []
        self.cjobs = self.cres = self.conf = None

    def add_chain(self, map_id, inst, w, slots, first=0, count=0, budget=-1, algo=ASTAR_EPS):
        n = len(inst["starts"])
        assert len(slots) == n
        self.specs.append(dict(kind="chain", map_id=map_id, inst=inst, w=w, slots=list(slots), first=first, count=count,
                               budget=budget, algo=algo, n_res=max(1, n - first)))
        return len(self.specs) - 1

    def add_job(self, map_id, inst, w, agent, ctx_paths=None, path_ids=None, path_len=None, vc=(), budget=-1, flags=0,
                result_path_id=-1):
        """An ordinary MRP_LL_ASTAR_EPS job of agent `agent`: the context shipped (ctx_paths: one [[x, y], ...] per agent, []
        = none) or named (path_ids + path_len, path_xy NULL)."""
        self.specs.append(dict(kind="job", map_id=map_id, inst=inst, w=w, agent=agent, ctx_paths=ctx_paths, path_ids=path_ids,
                               path_len=path_len, vc=[list(v) for v in vc], budget=budget, flags=flags,
                               result_path_id=result_path_id))
        return len(self.specs) - 1

    def _buffers(self, res):
        st = np.zeros((self.cap, 3), dtype=np.int32)
        ac = np.zeros(self.cap, dtype=np.int32)
        res.states_txy, res.actions, res.states_cap = st.ctypes.data_as(self.ll.I32P), ac.ctypes.data_as(self.ll.I32P), self.cap
        return st, ac

    def build(self):
        ll, I32P = self.ll, self.ll.I32P
        n = len(self.specs)
        self.cjobs, self.cres = (ll.mrp_ll_job * n)(), (ll.mrp_ll_result * n)()
        self.conf = (ll.mrp_ll_conflict * n)()
        for c in self.conf:
            for k, _ in ll.mrp_ll_conflict._fields_:
                setattr(c, k, -2)
        arr = lambda v, shape: np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(shape))  # noqa: E731
        for i, s in enumerate(self.specs):
            j, r, inst = self.cjobs[i], self.cres[i], s["inst"]
            j.map_id, j.algo, j.w, j.max_expansions = s["map_id"], s.get("algo", ASTAR_EPS), s["w"], s["budget"]
            s["bufs"] = self._buffers(r)
            if s["kind"] == "chain":
                sg = arr([a + b for a, b in zip(inst["starts"], inst["goals"])], (-1, 4))
                ids = arr(s["slots"], (-1,))
                sub = (ll.mrp_ll_result * s["n_res"])()
                for q in sub:  # what a result the engine does not write would still hold
                    q.status, q.cost, q.fmin, q.n_states, q.expanded, q.tier = -7, -7, -7, -7, -7, -7
                s["sub"], s["sub_bufs"] = sub, [self._buffers(q) for q in sub]
                j.flags, j.agent_idx, j.n_agents, j.chain_count = JOB_ROOT_CHAIN, s["first"], len(inst["starts"]), s["count"]
                j.chain_starts_goals_xy, j.path_ids = sg.ctypes.data_as(I32P), ids.ctypes.data_as(I32P)
                r.chain_results = ctypes.cast(sub, ctypes.c_void_p)
                self.keep.append((sg, ids))
                continue
            a = s["agent"]
            j.agent_idx, j.flags, j.result_path_id = a, s["flags"], s["result_path_id"]
            j.start_x, j.start_y = inst["starts"][a]
            j.goal_x, j.goal_y = inst["goals"][a]
            vc = arr(s["vc"], (-1, 3))
            j.n_vertex_constraints, j.vertex_constraints = len(vc), vc.ctypes.data_as(I32P)
            self.keep.append(vc)
            if s["path_ids"] is not None:
                ids, plen = arr(s["path_ids"], (-1,)), arr(s["path_len"], (-1,))
                j.n_agents, j.path_ids, j.path_len = len(ids), ids.ctypes.data_as(I32P), plen.ctypes.data_as(I32P)
                self.keep.append((ids, plen))
            elif s["ctx_paths"] is not None:
                plen = arr([len(p) for p in s["ctx_paths"]], (-1,))
                parr = [arr(p, (-1, 2)) for p in s["ctx_paths"]]
                pptr = (I32P * len(parr))(*[p.ctypes.data_as(I32P) for p in parr])
                j.n_agents, j.path_len, j.path_xy = len(parr), plen.ctypes.data_as(I32P), ctypes.cast(pptr, ctypes.POINTER(I32P))
                self.keep.append((plen, parr, pptr))
        return self

    @staticmethod
    def _record(r, bufs):
        st, ac = bufs
        m = r.n_states if r.status == OK else 0
        return dict(status=r.status, cost=r.cost, fmin=r.fmin, n_states=r.n_states, expanded=r.expanded, tier=r.tier,
                    states=st[:m].tolist(), actions=ac[:max(m - 1, 0)].tolist())

    def result(self, i):
        """The record of job i; a chain's has `chain`: the records of its agents."""
        s = self.specs[i]
        rec = self._record(self.cres[i], s["bufs"])
        if s["kind"] == "chain":  # (its n_states counts results, not states)
            rec.update(states=[], actions=[], chain=[self._record(q, b) for q, b in zip(s["sub"], s["sub_bufs"])])
        return rec

    def conflict(self, i):
        return {k: getattr(self.conf[i], k) for k, _ in self.ll.mrp_ll_conflict._fields_}
