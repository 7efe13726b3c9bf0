"""The corpus of tests/limit_cases.py, classified on the CPU: the conditions that keep tests/test_ll_limits_gpu.py from
hiding a failure — every class it asserts is populated, and hardly a case sits in the class that allows two answers."""
import collections
import time

import pytest

import limit_cases as lc

FAR = [254, 254]


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    t0 = time.perf_counter()
    cases = lc.corpus()
    return cases, time.perf_counter() - t0


def test_every_class_the_device_test_asserts_is_populated(corpus):
    cases, seconds = corpus
    n = collections.Counter((c["algo"], c["cls"], c["expect"]) for c in cases)
    print("class counts: " + ", ".join("%s/%s%s=%d" % (a, k, "/" + e if e else "", v) for (a, k, e), v in sorted(n.items(), key=str)))
    for algo in lc.ALGOS:
        assert n[(algo, "inside", None)] >= 20, (algo, n)
        assert n[(algo, "outside", "CAP_HORIZON")] >= 1, (algo, n)
    for algo in ("astar", "eps"):
        assert n[(algo, "outside", "CAP_NODES")] >= 1, (algo, n)
    for algo in ("eps", "eps_ta"):
        assert n[(algo, "outside", "CAP_FOCAL")] >= 3, (algo, n)
    between = sum(1 for c in cases if c["cls"] == "between")
    print("between: %d of %d cases; corpus built in %.1f s" % (between, len(cases), seconds))
    assert between <= 0.15 * len(cases), (between, len(cases))
    assert seconds < 60.0, seconds
    for c in cases:  # what the device test relies on
        assert c["engine"] in lc.ENGINES and (c["cls"] == "outside") == (c["expect"] is not None), c["name"]
        assert c["map"]["dimx"] * c["map"]["dimy"] <= lc.ENGINES[c["engine"]]["max_cells"], c["name"]


def test_the_edges_the_issue_names_are_in_their_classes(corpus):
    cases, _ = corpus
    by = {c["name"]: c for c in cases}
    inside = [c for c in cases if c["cls"] == "inside"]
    # cell (254, 254) as a goal and as a constraint, found and exact
    assert any(c["goal"] == FAR and c["ref"]["success"] for c in inside)
    assert any(c["goal"] == FAR and any(v[1:] == FAR for v in c["vc"]) and c["ref"]["success"] for c in inside)
    assert any(c["goal"] != FAR and any(v[1:] == FAR for v in c["vc"]) and c["map"]["dimx"] == 255 and c["map"]["dimy"] == 255
               for c in inside)
    # every geometry of the issue is met by an exact case of every algorithm
    for dims in ((33, 31), (31, 33), (48, 48), (100, 37), (37, 100), (64, 64), (255, 1), (1, 255), (255, 3), (255, 255),
                 (31, 17), (17, 31), (32, 5), (1, 32), (1, 1)):
        for algo in lc.ALGOS:
            assert any((c["map"]["dimx"], c["map"]["dimy"]) == dims and c["algo"] == algo for c in inside), (dims, algo)
    # 255 x 255: the task-assignment searches have 8 and 10 time steps there; some cases inside them, some outside
    for algo, T in (("ta", 8), ("eps_ta", 10)):
        on = [c for c in cases if c["algo"] == algo and c["map"]["dimx"] * c["map"]["dimy"] == 65025]
        assert {c["T"] for c in on} == {T}
        assert any(c["cls"] == "inside" for c in on) and any(c["expect"] == "CAP_HORIZON" for c in on), algo
    # g and horizon: 1023 steps are exact, 1024 are CAP_HORIZON for all four algorithms
    assert by["horizon/d1023/astar"]["cls"] == "inside" and by["horizon/d1023/astar"]["ref"]["cost"] == 1023
    assert 5 * by["horizon/d1023/astar"]["ref"]["expanded"] + 6 <= 1 << 22
    assert by["horizon/d1023/ta"]["ref"]["expanded"] == 1024
    for algo in lc.ALGOS:
        assert by["horizon/d1024/" + algo]["expect"] == "CAP_HORIZON" and by["horizon/d1024/" + algo]["ref"]["cost"] == 1024
    assert by["horizon/d786_w1.3/eps"]["cls"] == "inside"
    assert lc._f32_floor(1.3, by["horizon/d786_w1.3/eps"]["ref"]["fmin"]) + 1 < 1024
    # f and h: all outside
    for d in (2044, 2046, 2078, 4000):
        for algo in ("ta", "eps_ta"):
            c = by["fields/h%d/%s" % (d, algo)]
            assert c["expect"] == "CAP_HORIZON" and c["ref"]["cost"] == d and c["heur"] == "device"
    # focalH: n * L on the goal node, exact up to 2047
    for n_agents, L, exact in lc.FOCAL_NL:
        for suffix in ("default/eps", "arena_only/eps", "arena_only/eps_ta"):
            c = by["focal/n%d_L%d_%s" % (n_agents, L, suffix)]
            assert (c["ref"]["cost"], c["ref"]["expanded"]) == (L, L + 1)
            assert lc._path_focal(c, c["ref"]["states"]) == n_agents * L
            assert (c["cls"], c["expect"]) == (("inside", None) if exact else ("outside", "CAP_FOCAL")), c["name"]
            assert (n_agents * L <= lc.FH_MAX) == exact
