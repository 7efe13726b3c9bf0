"""MRP_HL_DEVICE_CONSTRAINTS=1 on the MI355X: the CBS / ECBS session drivers with their agents' constraint sets in the
engine's device-resident store (mrp_ll_submit_sets) reproduce the oracle's whole-instance results — cost, makespan,
highLevelExpanded, lowLevelExpanded and every path — alone, together with MRP_HL_DEVICE_SCAN=1, with co-workers sharing an
engine's store, and with a store so small that most sets ship flat."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu


def _digest(paths):
    h = hashlib.sha256()
    for p in paths:
        h.update(("|" + ",".join("%d:%d" % (x, y) for x, y in p)).encode())
    return h.hexdigest()[:16]


CONFIGS = {
    "sets": ({"MRP_HL_CONS_SLOTS": "65536"}, 4),
    "sets_and_scan": ({"MRP_HL_CONS_SLOTS": "65536", "MRP_HL_DEVICE_SCAN": "1"}, 4),
    "co_workers": ({"MRP_HL_CONS_SLOTS": "65536", "MRP_HL_MAX_ENGINES": "2"}, 4),
    "few_slots_small_budget": ({"MRP_HL_CONS_SLOTS": "256", "MRP_HL_CONS_WORDS": "6"}, 2),
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_switch_on_gives_the_oracles_results(bench_instances, oracle_expected, monkeypatch, config):
    from libmultirobotplanning_amd import hl
    env, n_threads = CONFIGS[config]
    monkeypatch.setenv("MRP_HL_DEVICE_CONSTRAINTS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ecbs = [n for n in sorted(bench_instances) if "32by32" in n and oracle_expected[n]["ecbs_w1.3"]["rc"] == 1]
    ecbs = ecbs[::4] + ["map_8by8_obst12_agents16_ex0", "map_8by8_obst12_agents16_ex1"]  # deep trees among them
    cbs = [n for n in sorted(bench_instances) if "8by8" in n and oracle_expected[n]["cbs"]["rc"] == 1
           and oracle_expected[n]["cbs"]["ll"] < 60000]
    s = hl.BatchSolver(device=0, n_threads=n_threads, slots=512)
    try:
        for algo, key, names in ((hl.ECBS, "ecbs_w1.3", ecbs), (hl.CBS, "cbs", cbs)):
            res, stats = s.solve([bench_instances[n] for n in names], algo=algo, w=1.3)
            for n, r in zip(names, res):
                e = oracle_expected[n][key]
                assert (r["status"], r["cost"], r["makespan"], r["hl_expanded"], r["ll_expanded"], _digest(r["paths"])) == (
                    hl.SOLVED, e["cost"], e["makespan"], e["hl"], e["ll"], e["digest"]), (n, config)
            assert stats["solved"] == len(names)
            assert max(oracle_expected[n][key]["hl"] for n in names) > 50  # (conflict trees deep enough to chain sets)
    finally:
        s.close()
