"""MRP_LL_JOB_ROOT_CHAIN at the C ABI (include/mrp_ll.h) against the oracle: the chains of tests/root_chain_cases.py, every
expected value computed on the CPU (chain_model) before the device is touched, every comparison of integers and exact.
A chain is accepted only in a session of A*-epsilon jobs with a path store (host/ll_pack.h packJob): every test here opens
mrp_ll_session_begin_algo(MRP_LL_ASTAR_EPS, 32) on an engine of 64 slots, collects with mrp_ll_poll under a deadline and
ends the session in `finally`."""
import contextlib
import ctypes
import time

import pytest

import root_chain_cases as rc

pytestmark = pytest.mark.gpu

NSLOTS = 512     # path-store slots
DEADLINE_S = 60  # of one ticket


def _filler(n):
    """n agents that walk 25 steps up their own column of an empty 32 x 32 map: paths of 26 states, longer than any of a case."""
    return dict(dimx=32, dimy=32, obstacles=[], starts=[[i, 0] for i in range(n)], goals=[[i, 25] for i in range(n)])


# two agents that have to pass each other in a 8 x 2 map: at w = 1.3 the second one's search depends on the first one's path
# (ten expansions instead of seven) and cannot avoid it (one vertex conflict at t = 3)
PASS = dict(dimx=8, dimy=2, obstacles=[], starts=[[0, 0], [6, 0]], goals=[[6, 0], [0, 0]])
PASS_W = 1.3
WIDE = dict(dimx=33, dimy=4, obstacles=[], starts=[[0, 0], [32, 3]], goals=[[3, 0], [30, 3]])  # no map of a chain


class World:
    def __init__(self, ll):
        self.ll = ll
        self.eng = ll.LowLevelEngine(device=0, n_tickets=2, slots=64)
        self.maps = {}

    def map_of(self, inst):
        key = (inst["dimx"], inst["dimy"], tuple(map(tuple, inst["obstacles"])))
        if key not in self.maps:
            self.maps[key] = self.eng.upload_map(inst["dimx"], inst["dimy"], inst["obstacles"])
        return self.maps[key]

    def submit(self, batch, scan=False):
        batch.build()
        lib, h, n, t = self.eng._lib, self.eng._h, len(batch.specs), ctypes.c_int32(-1)
        if scan:
            self.eng._check(lib.mrp_ll_submit_scan(h, 0, n, batch.cjobs, batch.cres, batch.conf, ctypes.byref(t)), "mrp_ll_submit_scan")
        else:
            self.eng._check(lib.mrp_ll_submit(h, n, batch.cjobs, batch.cres, ctypes.byref(t)), "mrp_ll_submit")
        return t.value

    def collect(self, ticket):
        done, t0 = ctypes.c_int32(0), time.monotonic()
        while not done.value:
            self.eng._check(self.eng._lib.mrp_ll_poll(self.eng._h, ticket, ctypes.byref(done)), "mrp_ll_poll")
            assert time.monotonic() - t0 < DEADLINE_S, "no completion within %d s" % DEADLINE_S

    def run(self, batch, scan=False):
        self.collect(self.submit(batch, scan))
        return [batch.result(i) for i in range(len(batch.specs))]

    @contextlib.contextmanager
    def session(self, mixed=False):
        if mixed:
            self.eng.session_begin(16)
        else:
            self.eng.session_begin_algo(self.ll.ASTAR_EPS, 32)
        try:
            yield
        finally:
            self.eng.session_end()


class Slots:
    """Distinct path-store slot ranges for the chains of one ticket."""

    def __init__(self):
        self.next = 0

    def take(self, n):
        assert self.next + n <= NSLOTS, "more slots than the store has"
        self.next += n
        return list(range(self.next - n, self.next))


@pytest.fixture(scope="module")
def world(oracle_mod):
    from libmultirobotplanning_amd import ll
    w = World(ll)
    try:
        w.eng.path_store_reserve(NSLOTS)
        for c in rc.select_cases():  # every map before the first session
            w.map_of(c["inst"])
        for inst in (rc.break_case()[0], _filler(1), PASS, WIDE):
            w.map_of(inst)
        yield w
    finally:
        w.eng.close()


def _ctx_before(paths, a):
    return [paths[b] if b < a else [] for b in range(len(paths))]


def _chain_diff(got, model):
    """Where a chain's record differs from the model's: [] or [(agent or "job", fields)]."""
    out = []
    job = [k for k in ("n_states", "expanded", "cost", "fmin") if got[k] != model[k]] + (["status"] if got["status"] != rc.OK else [])
    if job:
        out.append(("job", job, {k: got[k] for k in job}, {k: model.get(k) for k in job}))
    if len(got["chain"]) != len(model["results"]):
        out.append(("results", len(got["chain"]), len(model["results"])))
    for a, (g, m) in enumerate(zip(got["chain"], model["results"])):
        d = rc.same(g, m) + (["tier"] if g["tier"] != 0 else [])
        if d:
            out.append((a, d))
    return out


def _pick(cases, hand=("n16", "n17")):
    """A few chains of every kind: one per class (from different shapes), a parked one, and the named hand-made ones."""
    out = []
    for i, cls in enumerate(rc.CLASSES):
        of = [c for c in cases if c["cls"] == cls]
        out.append(of[i % len(of)])
    out.append([c for c in cases if c["parked"] and c not in out][0])
    out += [c for c in cases if c["cls"] == "hand" and any(("hand/" + h) in c["name"] for h in hand)]
    assert len({c["name"] for c in out}) == len(out)
    return out


# ---- a, b: whole chains against the model and against ordinary jobs ------------------------------------------------------

@pytest.fixture(scope="module")
def whole(world):
    """Every selected chain with agent_idx = 0 in one ticket, and in the same session every agent of every chain as an ordinary
    MRP_LL_ASTAR_EPS job with the model's earlier paths shipped in path_xy, in a second."""
    cases = rc.select_cases()
    chains, jobs, slots, first_job = rc.Batch(), rc.Batch(), Slots(), []
    for c in cases:
        inst, n, mid = c["inst"], len(c["inst"]["starts"]), world.map_of(c["inst"])
        chains.add_chain(mid, inst, c["w"], slots.take(n))
        first_job.append(len(jobs.specs))
        for a in range(n):
            jobs.add_job(mid, inst, c["w"], a, ctx_paths=_ctx_before(c["model"]["paths"], a))
    with world.session():
        t1, t2 = world.submit(chains), world.submit(jobs)
        world.collect(t1)
        world.collect(t2)
    got = [chains.result(i) for i in range(len(cases))]
    ordinary = [[jobs.result(f + a) for a in range(len(c["inst"]["starts"]))] for c, f in zip(cases, first_job)]
    return cases, got, ordinary


def test_whole_chains_equal_the_model(whole):
    """Every agent's status, cost, fmin, expanded, n_states, states and actions, tier 0; the job's n_states = n, expanded = the
    sum, cost = the oracle's conflict count, fmin = the encoded first conflict or -1."""
    cases, got, _ = whole
    bad = []
    for c, g in zip(cases, got):
        d = _chain_diff(g, c["model"])
        print("%-40s %-30s parked=%d  count %d first %#x" % (c["name"], c["cls"], c["parked"], g["cost"], g["fmin"] & 0xFFFFFFFF))
        if d:
            bad.append((c["name"], c["cls"], d))
    assert not bad, bad


def test_chain_results_equal_ordinary_jobs(whole):
    """"Every filled-in result is exactly what the ordinary job for that agent would have returned", field by field."""
    cases, got, ordinary = whole
    for c, g, jobs in zip(cases, got, ordinary):
        assert len(g["chain"]) == len(jobs)
        for a, (x, y) in enumerate(zip(g["chain"], jobs)):
            assert x == y, (c["name"], a, x, y)
            assert rc.same(y, c["model"]["results"][a]) == [], (c["name"], a)


# ---- c: what the chain leaves in the path store ---------------------------------------------------------------------------

def test_the_path_store_holds_the_chains_paths(world, oracle_mod):
    """Each slot range first receives a chain of longer paths (26 states), then the chain under test: a stale tail or length
    would show in the jobs that follow.  For up to three agents k of each chain an ordinary job names every other path by
    path_ids (path_xy NULL) and carries one vertex constraint on k's old path: it must equal the oracle's answer with the
    model's paths shipped.  One of them per chain also scans (mrp_ll_submit_scan): the node's conflicts are the oracle's."""
    picked = _pick(rc.select_cases())
    slots = Slots()
    fill, under, follow, expect = rc.Batch(), rc.Batch(), rc.Batch(), []
    for c in picked:
        inst, w, n, paths = c["inst"], c["w"], len(c["inst"]["starts"]), c["model"]["paths"]
        s, mid = slots.take(n), world.map_of(c["inst"])
        fill.add_chain(world.map_of(_filler(1)), _filler(n), 1.0, s)
        under.add_chain(mid, inst, w, s)
        scanned = False
        for k in sorted({0, n // 2, n - 1}):
            if len(paths[k]) < 2:
                continue
            t = len(paths[k]) // 2
            vc = [[t] + paths[k][t]]
            ctx = [p if b != k else [] for b, p in enumerate(paths)]
            want = rc.plan(inst, w, k, ctx, left=rc.ORACLE_CAP, vc=vc)
            node = None
            if not scanned:
                node = oracle_mod.conflict_scan([p if b != k else [q[1:] for q in want["states"]] for b, p in enumerate(paths)]) \
                    if want["status"] == rc.OK else dict(found=-1)
            follow.add_job(mid, inst, w, k, path_ids=[s[b] if b != k else -1 for b in range(n)],
                           path_len=[len(p) if b != k else 0 for b, p in enumerate(paths)], vc=vc, budget=rc.ORACLE_CAP,
                           flags=0 if scanned else rc.JOB_SCAN_CONFLICTS)
            expect.append((c["name"], k, want, node))
            scanned = True
    with world.session():
        filled = world.run(fill)
        tested = world.run(under)
        after = world.run(follow, scan=True)
    for c, f, g in zip(picked, filled, tested):
        n = len(c["inst"]["starts"])
        assert (f["status"], f["n_states"]) == (rc.OK, n), c["name"]
        assert all(q["n_states"] == 26 > len(p) for q, p in zip(f["chain"], c["model"]["paths"])), c["name"]
        assert _chain_diff(g, c["model"]) == [], c["name"]
    assert len(expect) >= 2 * len(picked)
    for i, ((name, k, want, node), g) in enumerate(zip(expect, after)):
        assert rc.same(g, want) == [], (name, k, g, want)
        conf = follow.conflict(i)
        if node is None:
            assert set(conf.values()) == {-2}, (name, k, conf)  # not flagged: not written
        elif node["found"] == -1:
            assert conf["found"] == -1, (name, k, conf)
        else:
            assert conf == node, (name, k, conf, node)


# ---- d: chunks and resumption ---------------------------------------------------------------------------------------------

def test_chunks_and_resumption(world):
    """chain_count = k, then agent_idx = k once the first job has been collected: together the whole chain; neither scans (cost
    = fmin = -1); the first job's results k .. are MRP_LL_NOT_RUN with zeroed fields.  chain_count = n and chain_count > n are
    the unchunked chain, scan included.  Cuts: 1, n / 2, n - 1."""
    picked = _pick(rc.select_cases(), hand=("n16", "n17", "n1", "all_on_goal"))
    slots, head, tail, plan_ = Slots(), rc.Batch(), rc.Batch(), []
    for c in picked:
        inst, w, n, mid, whole_ = c["inst"], c["w"], len(c["inst"]["starts"]), world.map_of(c["inst"]), c["model"]
        for k in sorted({1, n // 2, n - 1} - {0, n}):
            s = slots.take(n)
            h = head.add_chain(mid, inst, w, s, count=k)
            t = tail.add_chain(mid, inst, w, s, first=k)
            plan_.append((c, k, h, t))
        for count in (n, n + 5):
            plan_.append((c, count, head.add_chain(mid, inst, w, slots.take(n), count=count), None))
        assert rc.chain_model(inst, w, count=n + 5) == whole_
    with world.session():
        heads = world.run(head)
        tails = world.run(tail)
    assert any(t is not None for _, _, _, t in plan_)
    for c, k, h, t in plan_:
        inst, w, n, whole_ = c["inst"], c["w"], len(c["inst"]["starts"]), c["model"]
        if t is None:
            assert _chain_diff(heads[h], whole_) == [], (c["name"], "count", k)
            continue
        m1 = rc.chain_model(inst, w, count=k)
        m2 = rc.chain_model(inst, w, first=k, prior_paths=whole_["paths"])
        assert (m1["cost"], m1["fmin"], m2["cost"], m2["fmin"]) == (-1, -1, -1, -1)
        assert m1["results"][:k] + m2["results"] == whole_["results"] and m1["results"][k:] == [rc.not_run()] * (n - k)
        assert _chain_diff(heads[h], m1) == [], (c["name"], "count", k)
        assert _chain_diff(tails[t], m2) == [], (c["name"], "first", k)
        assert heads[h]["n_states"] == k and tails[t]["n_states"] == n - k


# ---- e: the shared budget -------------------------------------------------------------------------------------------------

def test_the_shared_budget(world):
    """max_expansions = E_0 + ... + E_(k-1) + r for cuts k in 0, 1, n / 2, n - 1 and r in 0, 1, E_k - 1, E_k (E: the model's
    expansions).  r < E_k: agent k is left with r and comes back as the oracle's search with cap_expansions = r does —
    MRP_LL_CAP_EXPANSIONS with expanded = r + 1, also at r = 0 — and as the ordinary job with max_expansions = r does; the
    agents behind are NOT_RUN, the job's n_states is k + 1, cost = fmin = -1.  r = E_k: agent k is planned; the agent behind it
    starts with nothing left and ends at its first expansion (the model says so: it subtracts like the header), and only with
    k = n - 1 is the root complete and scanned."""
    picked = _pick(rc.select_cases(), hand=("n17", "all_on_goal"))
    with world.session():
        for c in picked:
            inst, w, n, mid, whole_ = c["inst"], c["w"], len(c["inst"]["starts"]), world.map_of(c["inst"]), c["model"]
            E = [r["expanded"] for r in whole_["results"]]
            batch, slots, runs = rc.Batch(), Slots(), []
            for k in sorted({0, 1, n // 2, n - 1} - {n}):
                for r in sorted({0, 1, E[k] - 1, E[k]}):
                    if not 0 <= r <= E[k]:
                        continue
                    ci = batch.add_chain(mid, inst, w, slots.take(n), budget=sum(E[:k]) + r)
                    ji = batch.add_job(mid, inst, w, k, ctx_paths=_ctx_before(whole_["paths"], k), budget=r)
                    runs.append((k, r, ci, ji))
            got = world.run(batch)
            for k, r, ci, ji in runs:
                what = (c["name"], "k", k, "r", r)
                model = rc.chain_model(inst, w, budget=sum(E[:k]) + r)
                assert _chain_diff(got[ci], model) == [], what
                assert got[ci]["chain"][k] == got[ji], what  # the ordinary job with what is left, every field
                assert model["results"][:k] == whole_["results"][:k], what
                if r < E[k]:
                    assert (got[ci]["n_states"], got[ci]["cost"], got[ci]["fmin"]) == (k + 1, -1, -1), what
                    assert (got[ci]["chain"][k]["status"], got[ci]["chain"][k]["expanded"]) == (rc.CAP_EXPANSIONS, r + 1), what
                    assert model["results"][k + 1:] == [rc.not_run()] * (n - k - 1), what
                else:
                    assert got[ci]["chain"][k]["status"] == rc.OK and model["results"][k] == whole_["results"][k], what
                    assert (got[ci]["cost"] >= 0) == (k == n - 1), what


# ---- f: the break in front of a search that outgrows the tier -------------------------------------------------------------

def test_the_chain_ends_in_front_of_a_search_that_outgrows_the_tier(world, oracle_mod):
    """rc.break_case() under mrp_ll_configure_tiers(lds_rows = 12): the narrow tier gives a search up at the pop of a node that
    is no goal at t > lds_rows - 2 (ll_jobs.h narrowMaxT, ll_compact.h compactSearch) — agent 3's 15-state path has such
    nodes, the agents in front of it expand nothing beyond t = 4 (both margins of the issue hold: w * cost + 2 < 12 < states).
    The chain returns agents 0 .. 2 exactly and 3 .. as NOT_RUN; agent 3 as an MRP_LL_JOB_HEAVY job that stores its result and
    a chain from agent 4 complete the root as the model computes it with the full context; a scanning job over the stored
    paths finds the root's conflicts, the first of which is with agent 3's path."""
    inst, w = rc.break_case()
    n, K, mid, eng = len(inst["starts"]), rc.BREAK_K, world.map_of(inst), world.eng
    whole_ = rc.chain_model(inst, w)
    paths, s = whole_["paths"], list(range(10, 10 + n))
    eng.configure_tiers(lds_rows=rc.BREAK_ROWS)
    try:
        with world.session():
            b1 = rc.Batch()
            b1.add_chain(mid, inst, w, s)
            (broken,) = world.run(b1)
            b2 = rc.Batch()
            b2.add_job(mid, inst, w, K, path_ids=[s[b] if b < K else -1 for b in range(n)],
                       path_len=[len(paths[b]) if b < K else 0 for b in range(n)], flags=rc.JOB_HEAVY | rc.JOB_STORE_RESULT,
                       result_path_id=s[K])
            (heavy,) = world.run(b2)
            b3 = rc.Batch()
            b3.add_chain(mid, inst, w, s, first=K + 1)
            (rest,) = world.run(b3)
            b4 = rc.Batch()
            b4.add_job(mid, inst, w, n - 1, path_ids=s[:n - 1] + [-1], path_len=[len(p) for p in paths[:n - 1]] + [0],
                       flags=rc.JOB_SCAN_CONFLICTS)
            (last,) = world.run(b4, scan=True)
    finally:
        eng.configure_tiers(lds_rows=64)
    # the break really happened: no budget, every agent has a path, and yet the chain stopped in front of agent K
    want = dict(whole_, results=whole_["results"][:K] + [rc.not_run()] * (n - K), n_states=K,
                expanded=sum(r["expanded"] for r in whole_["results"][:K]), cost=-1, fmin=-1)
    assert _chain_diff(broken, want) == [], broken
    assert rc.same(heavy, whole_["results"][K]) == [] and heavy["tier"] != 0, heavy
    assert _chain_diff(rest, rc.chain_model(inst, w, first=K + 1, prior_paths=paths)) == [], rest
    assert [r for r in rest["chain"]] and rc.same(last, whole_["results"][n - 1]) == []
    node = oracle_mod.conflict_scan(paths)
    assert b4.conflict(0) == node and (node["agent1"], node["count"]) == (K, whole_["cost"]) and whole_["cost"] >= 1


# ---- g: rejections ------------------------------------------------------------------------------------------------------

def test_a_rejected_chain_runs_nothing_and_touches_no_slot(world, oracle_mod):
    """A chain through a batch mrp_ll_submit outside a session, in a mixed session, on a 33 x 4 map, and with a slot id equal to
    the number of reserved slots: MRP_LL_BAD_JOB, n_states = 0, expanded = 0, cost = fmin = -1, every chain result NOT_RUN with
    zeroed fields.  The ordinary job of the same ticket — which names slot 0, written before, and whose search depends on that
    path — returns the oracle's answer, the engine's job counter advances by that job alone, and a later scanning job over
    slot 0 still finds the path there.  Every rejected chain names slot 0 as its first agent's."""
    eng = world.eng
    case = [c for c in rc.select_cases() if c["cls"] == "vertex"][0]
    n = len(case["inst"]["starts"])
    p0 = rc.plan(PASS, PASS_W, 0, [[], []])
    path0 = [q[1:] for q in p0["states"]]
    want1 = rc.plan(PASS, PASS_W, 1, [path0, []])
    assert want1 != rc.plan(PASS, PASS_W, 1, [[], []]), "the second agent's search depends on the stored path"
    node = oracle_mod.conflict_scan([path0, [q[1:] for q in want1["states"]]])
    pmid = world.map_of(PASS)
    with world.session():
        b = rc.Batch()
        b.add_job(pmid, PASS, PASS_W, 0, flags=rc.JOB_STORE_RESULT, result_path_id=0)
        assert rc.same(world.run(b)[0], p0) == []

    def variant(what, chain_inst, chain_w, slots):
        jobs0 = eng.stats()["jobs"]
        b = rc.Batch()
        b.add_chain(world.map_of(chain_inst), chain_inst, chain_w, slots)
        b.add_job(pmid, PASS, PASS_W, 1, path_ids=[0, -1], path_len=[len(path0), 0])
        chain, job = world.run(b)
        assert (chain["status"], chain["n_states"], chain["expanded"], chain["cost"], chain["fmin"]) == (rc.BAD_JOB, 0, 0, -1, -1), (what, chain)
        assert chain["chain"] == [dict(rc.not_run(), tier=0)] * len(chain_inst["starts"]), (what, chain["chain"])
        assert rc.same(job, want1) == [], (what, job)
        assert eng.stats()["jobs"] - jobs0 == 1, what
        b = rc.Batch()
        b.add_job(pmid, PASS, PASS_W, 1, path_ids=[0, -1], path_len=[len(path0), 0], flags=rc.JOB_SCAN_CONFLICTS)
        (later,) = world.run(b, scan=True)
        assert rc.same(later, want1) == [] and b.conflict(0) == node, (what, later, b.conflict(0))

    variant("batch", case["inst"], case["w"], list(range(n)))
    with world.session(mixed=True):
        variant("mixed session", case["inst"], case["w"], list(range(n)))
    with world.session():
        variant("33 x 4 map", WIDE, 1.0, [0, 1])
        variant("slot id == slots", case["inst"], case["w"], list(range(n - 1)) + [NSLOTS])
