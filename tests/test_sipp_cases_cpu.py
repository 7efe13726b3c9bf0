"""The corpus of tests/sipp_cases.py, classified on the CPU: the conditions that keep tests/test_sipp_limits_gpu.py from
hiding a failure — every class, tier, form and hand-over side it asserts is populated, no case is beyond two limits, and
every edge the corpus is built around is in the class it was built for."""
import collections
import time

import pytest

import sipp_cases as sc


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    t0 = time.perf_counter()
    cases = sc.corpus()
    return cases, time.perf_counter() - t0


def test_every_class_tier_and_group_is_populated(corpus):
    cases, seconds = corpus
    n = collections.Counter((c["group"], c["form"], c["cls"], c["expect"]) for c in cases)
    print("class counts: " + ", ".join("%s/%s/%s%s=%d" % (g, f, k, "/" + e if e else "", v)
                                       for (g, f, k, e), v in sorted(n.items(), key=str)))
    tiers = collections.Counter(c["tier"] for c in cases if c["form"] == "resident" and c["cls"] == "inside")
    near = collections.Counter(x for c in cases for x in (c["near"] or ()))
    dk = sum(1 for c in cases if c["ref"]["decrease_keys"] > 0)
    print("resident tiers: %r; next to a hand-over: %r; cases with decrease-key events: %d" % (dict(tiers), dict(near), dk))
    print("%d cases; corpus built in %.1f s" % (len(cases), seconds))
    assert seconds < 60.0, seconds
    assert 200 <= len(cases) <= 500
    for c in cases:   # what the device test relies on
        assert c["engine"] in sc.ENGINES and c["form"] in sc.FORMS and c["cls"] in ("inside", "outside"), c["name"]
        assert (c["cls"] == "outside") == (c["expect"] is not None), c["name"]   # classify() asserted: beyond exactly one limit
        assert c["expect"] in (None, "CAP_HORIZON", "CAP_NODES", "BAD_JOB"), c["name"]
        if c["cls"] == "inside":
            assert c["tier"] in (0, 1, 2, 3) and (c["form"] == "resident" or c["tier"] == 1), c["name"]
            assert c["ref"]["expanded"] <= 20000, c["name"]   # the low thousands: a test of a few seconds
        assert c["pre"] is None or c["form"] == "resident", c["name"]
    # tiers: at least 20 resident cases end in each of 0, 2 and 3; 3 on each side of each hand-over that can be approached
    for t in (0, 2, 3):
        assert sum(1 for c in cases if c["group"] == "tiers" and c["tier"] == t) >= 20, (t, tiers)
    for key in ("lds_nodes", "mix_open"):
        for side in ("below", "above"):
            assert near[(key, side)] >= 3, (key, side, near)
    assert dk >= 20, dk
    # geometry: every map in all three forms, exact
    for dims in sc.GEOMETRY_DIMS:
        for form in sc.FORMS:
            on = [c for c in cases if c["group"] == "geometry" and (c["map"]["dimx"], c["map"]["dimy"]) == dims and c["form"] == form]
            assert on and all(c["cls"] == "inside" for c in on), (dims, form)
            if dims != (1, 1):
                assert sum(1 for c in on if c["ref"]["success"]) >= 4, (dims, form)
                far = [dims[0] - 1, dims[1] - 1]
                assert any(c["goal"] == far and c["ref"]["success"] for c in on), (dims, form)
                assert any(c["goal"][1] == far[1] for c in on) and any(c["goal"][0] == far[0] for c in on)
                assert any(any(v[:2] == far for v in c["intervals"]) for c in on), (dims, form)
    # every limit has a case on each side, in every form it applies to
    for expect in ("CAP_HORIZON", "CAP_NODES", "BAD_JOB"):
        for form in ("job", "table"):
            assert n[("limits", form, "outside", expect)] >= 1, (expect, form, n)
    assert n[("limits", "resident", "outside", "CAP_HORIZON")] >= 1 and n[("limits", "resident", "outside", "BAD_JOB")] >= 1


def test_the_named_edges_are_in_their_classes(corpus):
    cases, _ = corpus
    by = {c["name"]: c for c in cases}

    def inside(name, **want):
        c = by[name]
        assert c["cls"] == "inside", (name, c["why"])
        for k, v in want.items():
            assert (c[k] if k in c and k != "ref" else c["ref"][k]) == v, (name, k, v, c["why"])
        return c

    def outside(name, expect, limit):
        c = by[name]
        assert (c["cls"], c["expect"]) == ("outside", expect) and c["why"].startswith(limit + ":"), (name, c["why"])
        return c
    for form in sc.FORMS:
        # arrival: 1023 is exact, 1024 is CAP_HORIZON, whatever max_horizon is
        inside("limits/arrival_1023_std/" + form, success=True, cost=1023, max_arrival=1023, raw_states=2)
        outside("limits/arrival_1024_std/" + form, "CAP_HORIZON", "arrival")
        # a successor that is merely generated: the reference's answer costs 1 and never uses it
        c = inside("limits/late_interval_1023/" + form, success=True, cost=1, max_arrival=1023)
        assert c["ref"]["expanded"] == 2
        c = outside("limits/late_interval_1024/" + form, "CAP_HORIZON", "arrival")
        assert c["ref"]["cost"] == 1 and c["ref"]["max_arrival"] == 1024
        inside("limits/t0_1023/" + form, success=True, cost=0)
        assert by["limits/t0_1023/" + form]["ref"]["states"] == [[1023, 0, 0]]
        outside("limits/t0_1024/" + form, "BAD_JOB", "start time")
        # raw path: max_horizon / 2 states are exact, one more is CAP_HORIZON
        for engine in ("std", "long"):
            half = sc.ENGINES[engine]["max_horizon"] // 2
            inside("limits/raw_path_%d_%s/%s" % (half, engine, form), success=True, raw_states=half, cost=half - 1)
            c = outside("limits/raw_path_%d_%s/%s" % (half + 1, engine, form), "CAP_HORIZON", "path")
            assert c["ref"]["raw_states"] == half + 1 and c["ref"]["max_arrival"] <= sc.G_MAX
        # the byte condition of the travelling table on 255 x 255: the resident form is exact on both sides
        c = inside("limits/table_bytes_fit/" + form, success=True)
        assert c["K"] + 2 * c["S"] == 254 and 4 * (32513 + c["K"] + 1 + 2 * c["S"]) == sc.TABLE_BYTES
        c = by["limits/table_bytes_over/" + form]
        assert c["K"] + 2 * c["S"] == 255
        if form == "resident":
            assert c["cls"] == "inside" and not c["travels"]
        else:
            outside("limits/table_bytes_over/" + form, "CAP_NODES", "table")
    inside("limits/arrival_1023_long/job", cost=1023)
    outside("limits/arrival_1024_long/job", "CAP_HORIZON", "arrival")
    for form in ("job", "table"):
        an = sc.ENGINES["small"]["arena_nodes"]
        a = inside("limits/nodes_exact/" + form, success=True, created=an)
        b = outside("limits/nodes_one_more_interval/" + form, "CAP_NODES", "nodes")
        c = outside("limits/nodes_one_more_step/" + form, "CAP_NODES", "nodes")
        assert b["ref"]["created"] == an + 1 and b["ref"]["expanded"] == a["ref"]["expanded"]
        assert c["ref"]["created"] > an and c["ref"]["expanded"] > a["ref"]["expanded"] and c["ref"]["cost"] == a["ref"]["cost"] + 1
        # the status-word condition: 64 cells + 960 safe intervals fill the 1024 words, 961 do not fit
        c = inside("limits/table_states_fit/" + form, success=True)
        assert 64 + c["S"] == 1024 and c["ref"]["max_intervals"] > 16
        c = outside("limits/table_states_over/" + form, "CAP_NODES", "table")
        assert 64 + c["S"] == 1025 and 4 * (32 + c["K"] + 1 + 2 * c["S"]) <= sc.TABLE_BYTES
    # the walk down the comb: every expanded node is on the path, the hand-overs happen on the way
    inside("tiers/comb3/walk/resident", success=True, tier=2, raw_states=254, expanded=254)
    inside("tiers/comb6/walk/resident", success=True, tier=3, raw_states=254, expanded=254)
    a, b = inside("limits/resident_bound_65534/resident", tier=0), inside("limits/resident_bound_65535/resident", tier=1)
    assert not a["travels"] and b["travels"] and a["ref"]["states"] == b["ref"]["states"] and a["ref"]["success"]
    # tables: the listed cell is generated (it sits next to the start) and the path goes through its last finite interval
    for n in sc.RESIDENT_LISTS + sc.LONG_LISTS:
        forms = sc.FORMS if n in sc.RESIDENT_LISTS else ("job", "table")
        names = ["tables/list%d/%s" % (n, f) for f in forms] + (["tables/list%d_delta/resident" % n] if n in sc.RESIDENT_LISTS else [])
        for name in names:
            c = inside(name, success=True, max_intervals=n)
            safe = sc.safe_from(sc.list_of(n))
            want = safe[len(safe) - 2 if n >= 3 else len(safe) - 1][0]
            assert [want, 1, 1] in c["ref"]["states"], (name, want, c["ref"]["states"])
            assert c["travels"] == (c["form"] != "resident"), name
    assert by["tables/list9_delta/resident"]["pre"] == 1
    for form in sc.FORMS:
        inside("tables/adjacent/" + form, success=True, max_intervals=2)
        assert sc.safe_from([[2, 4], [5, 7]]) == [[0, 1], [8, sc.INT_MAX]]
        inside("tables/from_zero/" + form, success=True, cost=7)
        inside("tables/start_blocked_forever/" + form, success=False, expanded=0)
        c = inside("tables/goal_blocked_forever/" + form, success=False)
        assert c["ref"]["expanded"] > 1
        inside("tables/passage_blocked_forever/" + form, success=False, expanded=3, created=3)   # the start's column, no more
        inside("tables/t0_inside_collision/" + form, success=False, expanded=0)
        inside("tables/unsorted/" + form, success=True, max_intervals=4)
    # the later list wins: with [0, 3] alone L opens at 4; the earlier list [5, 9] would have delayed the arrival
    c = inside("tables/location_twice/job", success=True, max_intervals=1)
    assert [4, 1, 1] in c["ref"]["states"] and sc.cell_lists(c)[(1, 1)] == [[0, 3]]
    for name in ("tables/start_blocked_forever/resident", "tables/t0_inside_collision/resident", "geometry/1x1/blocked_at_t0/resident"):
        assert by[name]["tier"] == 1   # the job ends before its search: result.tier keeps its initial value
    assert inside("geometry/1x1/stay/resident", success=True, cost=0)["tier"] == 0
    assert inside("geometry/1x1/interval_ends/job", success=False, expanded=1)
