"""tests/ta_tier_cases.py on the CPU: the corpus holds what it is meant to hold (both sides of every edge of the LDS tier of
MRP_LL_ASTAR_TA, decrease-key searches of every wanted kind), every case has exactly one class, and the classifier — the
documented rule applied to the reference's trajectory — agrees with compactSearchTA itself, run through the wave emulator
under the case's limits: it hands over exactly when the rule says so, and equals the oracle bit for bit otherwise."""
import collections

import pytest

import ta_tier_cases as tc
from test_compact_emu import _emu_lib, emu_search_ta


@pytest.fixture(scope="module")
def cases(oracle_mod):
    return tc.corpus(oracle_mod)


def _by(cases, group):
    return [c for c in cases if c["group"] == group]


def test_every_case_has_one_class_and_one_reason(cases):
    for c in cases:
        assert c["cls"] in ("tier", "handed_over") and (c["cls"] == "tier") == (c["why"] == "fits"), c["name"]
        assert c["why"] in ("shape", "off", "h_start", "open", "time", "field", "fits"), c["name"]
        # quick on the device: 1500 expansions; 2000 for the rare decrease-key events beyond 768 open entries, 2800 for the
        # one search found that rediscovers a state in the fourth scan group (scripts/hunt_ta_decrease_keys.py --deep)
        limit = 2800 if c["name"].startswith("dk_deep") else 2000 if c["ref"]["open_at_decrease_key_max"] > 768 else 1500
        assert c["ref"]["expanded"] <= limit, c["name"]
    count = collections.Counter((c["group"], c["cls"]) for c in cases)
    for group in ("time", "rows", "open", "open_cap", "constraints", "field", "side"):
        assert count[(group, "tier")] > 0 and count[(group, "handed_over")] > 0, (group, count)


def test_counters_leave_the_answer_alone(oracle_mod, cases):
    for c in cases[::7]:
        plain = oracle_mod.ta_ll_search(c["map"], c["start"], c["goal"], c["vc"], c["ec"], cap_expansions=c["cap"], cap=tc.PATH_CAP)
        assert all(plain[k] == c["ref"][k] for k in plain), c["name"]
        assert set(c["ref"]) - set(plain) == set(oracle_mod.TA_COUNTERS)


def test_time_edge(cases):
    """A path whose last state has time 62 still finishes in the tier; 63 and beyond is handed over."""
    seen = collections.Counter()
    for c in _by(cases, "time"):
        last = c["ref"]["states"][-1][0]
        assert c["ref"]["max_time_expanded"] == last - 1, c["name"]
        assert (c["cls"], c["why"]) == (("tier", "fits") if last <= 62 else ("handed_over", "time")), (c["name"], last)
        seen[last] += 1
    assert all(seen[t] >= 3 for t in (61, 62, 63, 64)), seen
    # every form of the group on both sides: corner starts with 0 .. 3 forced Waits, a goal constraint, no task
    for prefix in ("time_corner", "time_goal", "time_notask"):
        assert {c["cls"] for c in _by(cases, "time") if c["name"].startswith(prefix)} == {"tier", "handed_over"}, prefix
    assert {len(c["vc"]) // 2 for c in _by(cases, "time") if c["name"].startswith("time_corner") and c["ref"]["states"][-1][0] in (62, 63)} == {0, 1, 2, 3}
    rows = _by(cases, "rows")
    assert len(rows) == 2 * sum(c["cls"] == "tier" for c in _by(cases, "time")) >= 40
    for a, b in zip(rows[::2], rows[1::2]):  # lds_rows = E + 2, then E + 1: only the tier flips
        E = a["ref"]["max_time_expanded"]
        assert a["ref"] == b["ref"] and (a["cfg"]["lds_rows"], b["cfg"]["lds_rows"]) == (E + 2, E + 1)
        assert (a["cls"], b["cls"], b["why"]) == ("tier", "handed_over", "time"), a["name"]


def test_open_list_edge(cases):
    M = {c["name"]: c["ref"]["max_open_at_pop"] for c in _by(cases, "open")}
    edge = tc.OPEN_MAX - tc.OPEN_ROOM
    below = max(m for m in M.values() if m <= edge)
    above = min(m for m in M.values() if m > edge)
    assert edge - 2 <= below and above <= edge + 2, (below, above)  # the closest pair the family gives: 1018 / 1020
    for c in _by(cases, "open"):
        assert (c["cls"] == "tier") == (M[c["name"]] <= edge) and c["why"] in ("fits", "open"), c["name"]
    assert M["open_flood_20_20_T59"] > 1023
    caps = _by(cases, "open_cap")
    assert len(caps) == 6
    for a, b in zip(caps[::2], caps[1::2]):
        m = a["ref"]["max_open_at_pop"]
        assert a["ref"] == b["ref"]
        assert (tc.open_cap(a["cfg"]), tc.open_cap(b["cfg"])) == (m + 5, m + 3)  # M + 4 is odd: the engine keeps M + 3
        assert (a["cls"], b["cls"], b["why"]) == ("tier", "handed_over", "open")


def test_constraint_field_and_side_groups(cases):
    for c in _by(cases, "constraints"):
        nv, ne = tc.packed_keys(c)
        assert (nv, ne) == (len(c["vc"]), len(c["ec"]))
        assert c["ref"]["cost"] == 6, c["name"]  # 5 without the last listed constraint
        assert (c["cls"] == "tier") == (nv <= 64 and ne <= 64)
    assert sorted(tc.packed_keys(c) for c in _by(cases, "constraints")) == [
        (0, 63), (0, 64), (0, 65), (63, 0), (64, 0), (64, 64), (64, 65), (65, 0)]
    field = {c["name"]: c for c in _by(cases, "field")}
    for h in tc.SNAKE_H:
        free, capped = field["field_h%d" % h], field["field_h%d_cap10" % h]
        assert free["ref"]["h_start"] == h == free["ref"]["cost"] and free["cls"] == "handed_over"
        assert capped["ref"]["rc"] == -1 and capped["ref"]["expanded"] == 11
        want = ("tier", "fits") if h <= 252 else ("handed_over", "field") if h <= 254 else ("handed_over", "h_start")
        assert (capped["cls"], capped["why"]) == want, (h, capped["why"])
    side = _by(cases, "side")
    assert [(c["map"]["dimx"], c["map"]["dimy"], c["cls"]) for c in side] == [
        (32, 32, "tier"), (33, 32, "handed_over"), (32, 33, "handed_over")]
    assert all(c["ref"]["states"] == side[0]["ref"]["states"] for c in side)


def test_decrease_key_conditions(cases):
    dk = _by(cases, "decrease_key")
    assert all(c["ref"]["decrease_keys"] > 0 for c in dk)
    assert len(dk) >= 12
    assert sum(c["ref"]["open_at_decrease_key_max"] > 256 for c in dk) >= 3
    assert sum(c["ref"]["decrease_keys"] >= 2 for c in dk) >= 3
    assert sum(c["ref"]["reparented_on_path"] > 0 for c in dk) >= 1
    assert sum(c["cls"] == "tier" for c in dk) >= 12  # ... and in the tier: compactSearchTA's re-key, not only runTaArena's


def test_classifier_and_emulated_tier_agree(cases):
    """compactSearchTA under the case's open_cap / max_t: status 3 / 4 exactly for "handed_over", the oracle's answer
    otherwise; never a read or write outside the window."""
    L = _emu_lib()
    done = collections.Counter()
    for c in cases:
        if not c["emulable"]:
            assert c["why"] in ("shape", "off"), c["name"]
            continue
        o = c["ref"]
        r = emu_search_ta(L, c["map"], c["start"], c["goal"], c["vc"], c["ec"], max_exp=c["cap"],
                          open_cap=tc.open_cap(c["cfg"]), max_t=tc.max_t(c["cfg"]))
        assert r["oob_reads"] == 0 and r["oob_writes"] == 0, c["name"]
        assert (r["status"] in (3, 4)) == (c["cls"] == "handed_over"), (c["name"], c["why"], r["status"])
        done[c["cls"]] += 1
        if c["cls"] == "handed_over":
            assert r["status"] == (3 if c["why"] == "open" else 4), (c["name"], c["why"], r["status"])
            continue
        if o["rc"] == -1:
            assert (r["status"], r["expanded"]) == (2, o["expanded"]), c["name"]
            continue
        assert (r["status"], r["expanded"], r["cost"], r["fmin"]) == (0, o["expanded"], o["cost"], o["fmin"]), c["name"]
        assert r["states"] == [s[1:] for s in o["states"]], c["name"]
    assert done["tier"] >= 90 and done["handed_over"] >= 50, done
    # an exact open cap of M + 4 — which no lds_nodes gives — through the emulator alone
    for c in _by(cases, "open_cap")[::2]:
        m = c["ref"]["max_open_at_pop"]
        r = emu_search_ta(L, c["map"], c["start"], c["goal"], c["vc"], c["ec"], open_cap=m + 4)
        assert r["status"] == 3, c["name"]


def test_classes_on_other_engines(cases):
    """with_cfg(): what the device test expects of engines whose tier is off."""
    for c in cases:
        for cfg in (dict(lds_nodes=-1), dict(arena_nodes=4095), dict(lds_path_bytes=1024)):
            assert tc.with_cfg(c, **cfg) == ("handed_over", "shape" if c["why"] == "shape" else "off")
        if c["cfg"] == tc.DEFAULT_CFG:
            assert tc.with_cfg(c, arena_nodes=4096) == (c["cls"], c["why"])
