"""The sequential restatement of CBS with task assignment (tests/support/cbs_ta_tree_check.cpp: cbs_ta.hpp:87-214 with the
Environment's assignment bookkeeping, over the oracle's low level) against what is known without it: the reference's own
test answers, and optimality — its cost is the minimum of the fixed-assignment conflict tree (oracle.ta_cbs_fixed) over
all assignments of maximum cardinality, which does not depend on any tie order."""
import itertools

import cbs_ta_corpus as corpus


def _assignments(inst):
    """Every assignment of distinct own potential goals that gives a task to as many agents as possible."""
    choices = [[None] + [tuple(g) for g in dict.fromkeys(map(tuple, pg))] for pg in inst["potential_goals"]]
    best, out = -1, []
    for combo in itertools.product(*choices):
        used = [c for c in combo if c is not None]
        if len(set(used)) != len(used):
            continue
        if len(used) > best:
            best, out = len(used), []
        if len(used) == best:
            out.append([list(c) if c is not None else None for c in combo])
    return out


def test_reference_inputs_costs_and_end_states(ref_tests):
    """test/test_cbs_ta.py:24-38: costs 6, 6, 5; a2: agent0 ends at x 4, y 0, t 4 and agent1 at (2, 1); a3: agent0 at 3, 0, 3."""
    got = {n: corpus.reference(i) for n, i in corpus.ref_inputs(ref_tests).items()}
    assert {n: r["cost"] for n, r in got.items()} == ref_tests["cbs_ta"]["cost"] == dict(
        mapfta_simple1_a1=6, mapfta_simple1_a2=6, mapfta_simple1_a3=5)
    assert all(r["status"] == 0 and r["num_task_assignments"] >= 1 for r in got.values())
    assert got["mapfta_simple1_a2"]["ends"][0] == [4, 0, 4] and got["mapfta_simple1_a2"]["ends"][1][:2] == [2, 1]
    assert got["mapfta_simple1_a3"]["ends"][0] == [3, 0, 3]


def test_cost_is_the_minimum_over_all_assignments(oracle_mod):
    insts = corpus.corpus()
    assert len(insts) == 40
    refs = [corpus.reference(i) for i in insts]
    for seed, inst, r in zip(corpus.SEEDS, insts, refs):
        m = dict(dimx=inst["dimx"], dimy=inst["dimy"], obstacles=inst["obstacles"])
        costs = []
        for tasks in _assignments(inst):
            if not any(t is not None for t in tasks):
                continue
            summary, _ = oracle_mod.ta_cbs_fixed(m, inst["starts"], tasks)
            if summary["solved"]:
                costs.append(summary["cost"])
        if costs:
            assert r["status"] == 0 and r["cost"] == min(costs), (seed, r["cost"], sorted(costs)[:3])
        else:
            assert r["status"] == 1, seed
    # the corpus reaches what it is for
    assert sum(1 for r in refs if r["root_conflicts"] > 0) * 3 >= len(refs)
    assert sum(1 for r in refs if r["n_roots"] >= 3) >= 5
    assert any(len({tuple(g) for gs in i["potential_goals"] for g in gs}) < len(i["starts"]) for i in insts)  # more agents than goals
