"""MRP_LL_ASTAR_TA on the MI355X at the hand-overs between its two tiers and in its decrease-key branches: the corpus of
tests/ta_tier_cases.py through the C ABI, every case against the oracle word for word (status, cost, fmin, expanded,
states, actions, action costs) and result.tier against the classifier (0 for "tier", 1 for "handed_over") — in batches
(the A*-only kernels and, with one A*-epsilon job added, the mixed kernel), in a mixed session, in an A* session, under
the lds_nodes / lds_rows pairs of the corpus, and on engines whose LDS tier is off (lds_nodes = -1, an arena slot one node
short of the tier's cameFrom table, lds_path_bytes below 2048): compactSearchTA's re-key and runTaArena's see the same
decrease-key searches and must give the same words."""
import collections

import pytest

import ta_tier_cases as tc

pytestmark = pytest.mark.gpu

CHUNK = 96  # jobs per call: below every engine's slots and every session's ring


@pytest.fixture(scope="module")
def cases(oracle_mod):
    return tc.corpus(oracle_mod)


class _Engine:
    """One LowLevelEngine with the corpus' maps and tables uploaded once (they cannot be uploaded during a session)."""

    def __init__(self, cases, **options):
        from libmultirobotplanning_amd import ll
        self.ll = ll
        self.eng = ll.LowLevelEngine(device=0, n_tickets=1, slots=128, **options)
        self.maps, self.heurs = {}, {}
        for c in cases:
            self._ids(c)

    def _ids(self, c):
        m = c["map"]
        key = id(m)
        if key not in self.maps:
            self.maps[key] = self.eng.upload_map(m["dimx"], m["dimy"], m["obstacles"])
        if c["goal"] is None:
            return self.maps[key], -1
        hk = (key, tuple(c["goal"]))
        if hk not in self.heurs:
            self.heurs[hk] = self.eng.upload_heuristic(self.maps[key], tc.bfs_table(m["dimx"], m["dimy"], m["obstacles"], c["goal"]))
        return self.maps[key], self.heurs[hk]

    def job(self, c):
        mid, hid = self._ids(c)
        return self.ll.LLJob(map_id=mid, algo=self.ll.ASTAR_TA, start=c["start"], goal=c["goal"], vertex_constraints=c["vc"],
                             edge_constraints=c["ec"], max_expansions=c["cap"], heuristic_id=hid)

    def run(self, cases, classes=None, extra=None):
        """`cases` in calls of CHUNK jobs; classes: name -> (cls, why) on this engine as it is configured now (default:
        the case's own).  extra: (job, check) of another algorithm that rides along in every call.  Returns the number
        of searches per tier."""
        ll = self.ll
        tiers = collections.Counter()
        for i in range(0, len(cases), CHUNK):
            part = cases[i:i + CHUNK]
            jobs = [self.job(c) for c in part] + ([extra[0]] if extra else [])
            res = self.eng.search_batch(jobs)
            if extra:
                extra[1](res.pop())
            for c, r in zip(part, res):
                o = c["ref"]
                cls, why = classes[c["name"]] if classes else (c["cls"], c["why"])
                where = (c["name"], cls, why)
                if o["rc"] == -1:
                    assert (r.status, r.expanded) == (ll.CAP_EXPANSIONS, o["expanded"]), where
                else:
                    assert (r.status, r.cost, r.fmin, r.expanded) == (ll.OK, o["cost"], o["fmin"], o["expanded"]), where
                    assert r.states == o["states"], where
                    assert (r.actions, r.action_costs) == (o["actions"], o["action_costs"]), where
                assert r.tier == (0 if cls == "tier" else 1), where + (r.tier,)
                tiers[r.tier] += 1
        return tiers

    def close(self):
        self.eng.close()


def _default(cases):
    return [c for c in cases if c["cfg"] == tc.DEFAULT_CFG]


def _classes(cases, **cfg):
    return {c["name"]: tc.with_cfg(c, **cfg) for c in cases}


def test_batches_and_sessions_of_the_default_engine(cases, oracle_mod):
    """The whole corpus at the default limits through the four ways a task-assignment job reaches a kernel."""
    E = _Engine(cases)
    ll = E.ll
    try:
        mine = _default(cases)
        want = collections.Counter(0 if c["cls"] == "tier" else 1 for c in mine)
        assert want[0] >= 60 and want[1] >= 30
        assert E.run(mine) == want                                  # task-assignment jobs only: the A*-only kernels
        m = tc.EMPTY32
        o = oracle_mod.ll_search(oracle_mod.ASTAR_EPS, m, 0, [2, 3], [9, 11], w=1.3)
        eps = ll.LLJob(map_id=E.maps[id(m)], algo=ll.ASTAR_EPS, start=[2, 3], goal=[9, 11], w=1.3)

        def check_eps(r):
            assert (r.status, r.cost, r.fmin, r.expanded, r.states) == (ll.OK, o["cost"], o["fmin"], o["expanded"], o["states"])
        assert E.run(mine, extra=(eps, check_eps)) == want          # one A*-epsilon job added: the mixed kernel
        E.eng.session_begin(64)                                     # a mixed session
        try:
            assert E.run(mine) == want
            assert E.run(mine[:CHUNK - 1], extra=(eps, check_eps))[0] > 0
        finally:
            E.eng.session_end()
        E.eng.session_begin_algo(ll.ASTAR, 64)                      # an A* session takes these jobs too
        try:
            assert E.run(mine) == want
        finally:
            E.eng.session_end()
    finally:
        E.close()


def test_lds_nodes_and_lds_rows_pairs_on_one_engine(cases):
    """mrp_ll_configure_tiers' lds_rows = E + 2 / E + 1 and lds_nodes for an open cap of M + 5 / M + 4: one side finishes
    in the tier, the other is handed over, the words are the same."""
    mine = [c for c in cases if c["group"] in ("rows", "open_cap")]
    by_cfg = collections.defaultdict(list)
    for c in mine:
        by_cfg[(c["cfg"]["lds_nodes"], c["cfg"]["lds_rows"])].append(c)
    E = _Engine(mine)
    try:
        tiers = collections.Counter()
        for (nodes, rows), part in sorted(by_cfg.items()):
            E.eng.configure_tiers(lds_nodes=nodes or tc.LDS_NODES_MAX, lds_rows=rows or 64)
            tiers += E.run(part)
        assert tiers[0] == tiers[1] == len(mine) // 2 >= 30
        # back at the defaults the tier finishes every one of them
        E.eng.configure_tiers(lds_nodes=tc.LDS_NODES_MAX, lds_rows=64)
        assert E.run(mine, classes=_classes(mine, lds_nodes=0, lds_rows=0)) == {0: len(mine)}
    finally:
        E.close()


def test_arena_tier_alone_rekeys_the_same(cases):
    """lds_nodes = -1: runTaArena's decrease-key on the searches compactSearchTA's is tested with, and the time group."""
    mine = [c for c in _default(cases) if c["group"] in ("decrease_key", "time")]
    assert sum(c["ref"]["decrease_keys"] > 0 for c in mine) >= 12
    E = _Engine(mine, lds_nodes=-1)
    try:
        assert E.run(mine, classes=_classes(mine, lds_nodes=-1)) == {1: len(mine)}
    finally:
        E.close()


def _fits_small_arena(c):
    """runTaArena in a slot of 4094 nodes: its status table is the room of two heap arrays (16384 words), one word per
    (time step, cell), and it wants the time step after the last one it expands."""
    cells = c["map"]["dimx"] * c["map"]["dimy"]
    return cells * (c["ref"]["max_time_expanded"] + 3) <= 16384 and c["ref"]["created"] + 5 <= 4000


@pytest.mark.parametrize("arena_nodes", [4096, 4095])
def test_arena_slot_that_just_holds_the_parent_table(cases, arena_nodes):
    """arena_nodes = 4096: the tier's 64 KiB cameFrom table fills the slot's node area exactly, the tier is on; 4095 (kept
    as 4094): one record short, every search runs in the arena tier.  mrp_ll_create accepts both."""
    mine = [c for c in _default(cases) if _fits_small_arena(c)]
    assert sum(c["ref"]["decrease_keys"] > 0 for c in mine) >= 8 and any(c["why"] == "shape" for c in mine)
    E = _Engine(mine, arena_nodes=arena_nodes)
    try:
        tiers = E.run(mine, classes=_classes(mine, arena_nodes=arena_nodes))
        if arena_nodes == 4096:
            assert tiers[0] >= 12 and tiers[1] >= 1
        else:
            assert tiers == {1: len(mine)}
    finally:
        E.close()


def test_path_table_room_below_the_tiers_minimum(cases):
    """configure_tiers(lds_path_bytes=1024) is accepted and turns the tier off for this search (runJobTA wants 2048)."""
    mine = [c for c in _default(cases) if c["group"] in ("decrease_key", "time", "constraints")]
    E = _Engine(mine)
    try:
        assert E.run(mine[:8])[0] > 0
        E.eng.configure_tiers(lds_path_bytes=1024)
        assert E.run(mine, classes=_classes(mine, lds_path_bytes=1024)) == {1: len(mine)}
    finally:
        E.close()
