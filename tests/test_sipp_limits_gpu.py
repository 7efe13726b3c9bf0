"""MRP_LL_SIPP on the MI355X at its tier hand-overs, table forms and loud limits: the corpus of tests/sipp_cases.py through
the C-ABI.  A case the reference proves to be inside the limits include/mrp_ll.h documents for MRP_LL_SIPP must come back
bit for bit — status, cost, fmin, expansions, states with their times, actions, action costs — and in the memory tier the
reference's trajectory puts it in (result.tier); a case it proves to be beyond exactly one limit must come back with that
limit's status and without a path.  There is no class that allows two answers.  A g that wraps at 1024, an interval
index that loses a bit on its way through a packed x word, a hand-over that drops a node record or a count word that is
not written yield a plausible wrong path, another expansion count or another tier, and fail here."""
import collections

import pytest

import sipp_cases as sc

pytestmark = pytest.mark.gpu
SLICE = 256   # resident jobs in flight (the session takes 512)


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    return sc.corpus()


@pytest.fixture(scope="module")
def engines():
    """name -> state of the engine with the option set sc.ENGINES[name], created on first use, every one closed when the
    module is done.  state: eng, maps (what has been uploaded), batch (group -> results of its job / table cases)."""
    from libmultirobotplanning_amd import ll
    made = {}

    def get(name):
        if name not in made:
            made[name] = dict(eng=ll.LowLevelEngine(device=0, **sc.ENGINES[name]), maps={}, batch={})
        return made[name]
    try:
        yield get
    finally:
        for st in made.values():
            st["eng"].close()


def _map_id(st, m):
    if id(m) not in st["maps"]:
        st["maps"][id(m)] = st["eng"].upload_map(m["dimx"], m["dimy"], m["obstacles"])
    return st["maps"][id(m)]


def _job(st, c, table=None):
    from libmultirobotplanning_amd import ll
    return ll.LLJob(map_id=_map_id(st, c["map"]), algo=ll.SIPP, start=c["start"], goal=c["goal"], initial_cost=c["t0"],
                    collision_intervals=c["intervals"] if table is None else (), sipp_table=table)


def _add(eng, h, ivs):
    for x, y, a, b in ivs:
        eng.sipp_table_add(h, x, y, a, b)


def _run_batch(st, cases):
    """job and table cases through mrp_ll_search_batch: every table travels whole."""
    eng = st["eng"]
    tabs, jobs = [], []
    try:
        for c in cases:
            h = None
            if c["form"] == "table":
                h = eng.sipp_table_create(_map_id(st, c["map"]))
                tabs.append(h)
                _add(eng, h, c["intervals"])
            jobs.append(_job(st, c, h))
        return eng.search_batch(jobs, states_cap=eng.max_horizon)
    finally:
        for h in tabs:
            eng.sipp_table_destroy(h)


def _run_resident(st, cases):
    """resident cases through one SIPP session, each on its own table (created before the session begins, as the maps are),
    SLICE jobs at a time.  A case with `pre` adds that many intervals, runs a warm-up job on the table (same start and
    goal), then adds the rest: they reach the device as a delta."""
    from libmultirobotplanning_amd import ll
    eng = st["eng"]
    tabs = [eng.sipp_table_create(_map_id(st, c["map"])) for c in cases]
    out = []
    try:
        eng.session_begin_sipp(32)
        try:
            for k in range(0, len(cases), SLICE):
                part = list(zip(cases[k:k + SLICE], tabs[k:k + SLICE]))
                for c, h in part:
                    _add(eng, h, c["intervals"] if c["pre"] is None else c["intervals"][:c["pre"]])
                warm = [(c, h) for c, h in part if c["pre"] is not None]
                if warm:
                    for r in eng.search_batch([_job(st, c, h) for c, h in warm], states_cap=eng.max_horizon):
                        assert r.status in (ll.OK, ll.NO_SOLUTION) and r.tier == 0, (r.status, r.tier)
                    for c, h in warm:
                        _add(eng, h, c["intervals"][c["pre"]:])
                out += eng.search_batch([_job(st, c, h) for c, h in part], states_cap=eng.max_horizon)
        finally:
            eng.session_end()
    finally:
        for h in tabs:
            eng.sipp_table_destroy(h)
    return out


def _key(r):
    return (r.status, r.cost, r.fmin, r.expanded, r.n_states, r.states, r.actions, r.action_costs, r.tier)


def _check(cases, res):
    """The class assertions of the module docstring.  Returns the counts per (form, class, status or tier)."""
    from libmultirobotplanning_amd import ll
    seen = collections.Counter()
    assert len(res) == len(cases)
    for c, r in zip(cases, res):
        o = c["ref"]
        tag = (c["name"], c["cls"], c["expect"], c["why"], "status", r.status, "expanded", r.expanded, o["expanded"], "tier", r.tier)
        if c["cls"] == "outside":
            assert r.status == getattr(ll, c["expect"]), tag
            assert r.n_states == 0 and r.states == [] and r.actions == [], tag
            seen[(c["form"], "outside", c["expect"])] += 1
            continue
        assert r.status == (ll.OK if o["success"] else ll.NO_SOLUTION), tag
        assert r.expanded == o["expanded"], tag
        if o["success"]:
            assert (r.cost, r.fmin, r.n_states) == (o["cost"], o["fmin"], len(o["states"])), (tag, r.cost, r.fmin, o["cost"], o["fmin"])
            assert r.states == o["states"], (tag, r.states, o["states"])
            assert r.actions == o["actions"] and r.action_costs == o["action_costs"], tag
        else:
            assert r.n_states == 0 and r.states == [], tag
        assert r.tier == c["tier"], tag
        seen[(c["form"], "inside", c["tier"])] += 1
    return seen


def _group(engines, corpus, group, forms=sc.FORMS):
    """Runs the group's cases of `forms`, engine by engine; returns (cases, results) in one order."""
    cases_all, res_all = [], []
    for name in sc.ENGINES:
        st = None
        batch = [c for c in corpus if c["group"] == group and c["engine"] == name and c["form"] in ("job", "table") and c["form"] in forms]
        if batch:
            st = engines(name)
            if group not in st["batch"]:
                st["batch"][group] = _run_batch(st, batch)
            cases_all += batch
            res_all += st["batch"][group]
        resident = [c for c in corpus if c["group"] == group and c["engine"] == name and c["form"] == "resident" and "resident" in forms]
        if resident:
            st = engines(name)
            cases_all += resident
            res_all += _run_resident(st, resident)
    return cases_all, res_all


def test_geometry_non_square_and_non_power_of_two_maps(engines, corpus):
    """33 x 31 to 255 x 255, one row, one column, three rows and three columns of 255, 7 x 5 and 1 x 1, in all three
    forms: goals on the last row, the last column and the last cell, collision intervals on those cells.  The cell / dimx
    of sippLoop, the y * dimx + x keys and the resident rows are only right here if they are right for every dimx."""
    cases, res = _group(engines, corpus, "geometry")
    seen = _check(cases, res)
    assert seen[("job", "inside", 1)] >= 50 and seen[("table", "inside", 1)] >= 50 and seen[("resident", "inside", 0)] >= 50, seen


def test_geometry_jobs_in_a_sipp_session_equal_batch_mode(engines, corpus):
    """The geometry group's job-form cases once more through the resident SIPP kernel (their tables travel with them):
    word for word what batch mode answered."""
    n = 0
    for name in sc.ENGINES:
        cases = [c for c in corpus if c["group"] == "geometry" and c["engine"] == name and c["form"] == "job"]
        if not cases:
            continue
        st = engines(name)
        if "geometry" not in st["batch"]:
            both = [c for c in corpus if c["group"] == "geometry" and c["engine"] == name and c["form"] in ("job", "table")]
            st["batch"]["geometry"] = _run_batch(st, both)
        both = [c for c in corpus if c["group"] == "geometry" and c["engine"] == name and c["form"] in ("job", "table")]
        want = [r for c, r in zip(both, st["batch"]["geometry"]) if c["form"] == "job"]
        eng = st["eng"]
        eng.session_begin_sipp(32)
        try:
            got = eng.search_batch([_job(st, c) for c in cases], states_cap=eng.max_horizon)
        finally:
            eng.session_end()
        for c, a, b in zip(cases, got, want):
            assert _key(a) == _key(b), (c["name"], a.status, b.status, a.expanded, b.expanded)
        n += len(cases)
    assert n >= 50


def test_tier_hand_overs(engines, corpus):
    """Resident searches that end in the LDS tier, in the middle tier and in the arena, at least 20 each, and the comb cases
    within 8 nodes / open entries of either hand-over on both sides: every one in the tier the reference's trajectory puts
    it in, and exact — the repacked node records, the rebuilt 64-bit open entries and their x word included."""
    cases, res = _group(engines, corpus, "tiers")
    seen = _check(cases, res)
    for tier in (0, 2, 3):
        assert seen[("resident", "inside", tier)] >= 20, seen
    near = collections.Counter(x for c in cases for x in c["near"])
    assert all(near[(k, s)] >= 3 for k in ("lds_nodes", "mix_open") for s in ("below", "above")), near


def test_table_shapes(engines, corpus):
    """Adjacent intervals, an interval from 0, cells blocked for ever, a start time inside a collision interval, unsorted
    lists, a location given twice, and lists of 1 to 15 (resident: the three record sizes, fresh and as a delta) and 16 to
    130 safe intervals (the one-motion-at-a-time branch and its second and third pass)."""
    cases, res = _group(engines, corpus, "tables")
    seen = _check(cases, res)
    assert seen[("resident", "inside", 0)] >= 20 and seen[("resident", "inside", 1)] == 2, seen
    assert seen[("job", "inside", 1)] >= 20 and seen[("table", "inside", 1)] >= 20, seen


def test_loud_limits(engines, corpus):
    """Arrival times 1023 / 1024 (also for a successor that is only generated), start times 1023 / 1024, raw paths of
    max_horizon / 2 states and one more, exactly arena_nodes nodes and one more, travelling tables that fill the slot and
    that miss it by one word (both conditions)."""
    cases, res = _group(engines, corpus, "limits")
    seen = _check(cases, res)
    for form in ("job", "table"):
        assert seen[(form, "outside", "CAP_HORIZON")] >= 4 and seen[(form, "outside", "CAP_NODES")] >= 4, seen
        assert seen[(form, "outside", "BAD_JOB")] == 1, seen
    assert seen[("resident", "outside", "CAP_HORIZON")] >= 4 and seen[("resident", "outside", "BAD_JOB")] == 1, seen


def test_resident_bound_shows_only_in_staged_bytes(engines, corpus):
    """A safe interval that starts at 65534 keeps its table on the device, one that starts at 65535 makes it travel whole:
    the same exact answer, tier 0 against 1, and a few words against the whole table in pinned memory."""
    by = {c["name"]: c for c in corpus}
    pair = [by["limits/resident_bound_%d/resident" % b] for b in (65534, 65535)]
    st = engines("std")
    eng = st["eng"]
    tabs = [eng.sipp_table_create(_map_id(st, c["map"])) for c in pair]
    res, staged = [], []
    try:
        eng.session_begin_sipp(32)
        try:
            for c, h in zip(pair, tabs):
                _add(eng, h, c["intervals"])
                b0 = eng.stats()["staged_bytes"]
                res += eng.search_batch([_job(st, c, h)], states_cap=eng.max_horizon)
                staged.append(eng.stats()["staged_bytes"] - b0)
        finally:
            eng.session_end()
    finally:
        for h in tabs:
            eng.sipp_table_destroy(h)
    seen = _check(pair, res)
    assert seen[("resident", "inside", 0)] == 1 and seen[("resident", "inside", 1)] == 1, seen
    cells = pair[1]["map"]["dimx"] * pair[1]["map"]["dimy"]
    table_bytes = 4 * ((cells + 1) // 2 + pair[1]["K"] + 1 + 2 * pair[1]["S"])
    print("staged bytes: resident %d, travelling %d (its table: %d)" % (staged[0], staged[1], table_bytes))
    assert staged[1] - staged[0] >= table_bytes - 256 and staged[0] < 1024, (staged, table_bytes)
