"""The sequential restatement of ECBS with task assignment (tests/support/ecbs_ta_tree_check.cpp: ecbs_ta.hpp:94-352 with the
Environment's assignment bookkeeping, over the checker's AStarEpsilon low level) against what is known without it: the
reference's own test answers at w = 1.0, optimality at w = 1.0 (the CBS-TA restatement's cost), the suboptimality bound at
every w, and returned paths without a conflict under example/ecbs_ta.cpp's getFirstConflict, restated here in Python."""
import cbs_ta_corpus
import ecbs_ta_tree_corpus as corpus


def _first_conflict(paths):
    """ecbs_ta.cpp:440-491: t < the longest STATE COUNT, paths held at their last cell, vertex pairs before edge pairs."""
    def at(p, t):
        return tuple(p[min(t, len(p) - 1)])
    for t in range(max(len(p) for p in paths)):
        for i in range(len(paths)):
            for j in range(i + 1, len(paths)):
                if at(paths[i], t) == at(paths[j], t):
                    return ("vertex", t, i, j)
        for i in range(len(paths)):
            for j in range(i + 1, len(paths)):
                if at(paths[i], t) == at(paths[j], t + 1) and at(paths[i], t + 1) == at(paths[j], t):
                    return ("edge", t, i, j)
    return None


def test_reference_inputs_costs_and_end_states(ref_tests):
    """test/test_ecbs_ta.py at w = 1.0: costs 6, 6, 5; a2: agent0 ends at x 4, y 0, t 4 and agent1 at (2, 1); a3: agent0 at
    3, 0, 3."""
    got = {n: corpus.reference(i, 1.0) for n, i in corpus.ref_inputs(ref_tests).items()}
    assert {n: r["cost"] for n, r in got.items()} == dict(mapfta_simple1_a1=6, mapfta_simple1_a2=6, mapfta_simple1_a3=5)
    assert all(r["status"] == 0 and r["num_task_assignments"] >= 1 for r in got.values())
    assert got["mapfta_simple1_a2"]["ends"][0] == [4, 0, 4] and got["mapfta_simple1_a2"]["ends"][1][:2] == [2, 1]
    assert got["mapfta_simple1_a3"]["ends"][0] == [3, 0, 3]


def test_optimal_at_w_1_bounded_above_it_and_free_of_conflicts(ref_tests):
    """At w = 1.0 both restatements are optimal: the cost equals CBS-TA's wherever CBS-TA has an answer (it gives up on an
    empty first assignment, cbs_ta.hpp:105-113, where ECBS-TA plans the agents without tasks).  At every w the cost is at most
    w times the w = 1.0 cost."""
    insts = corpus.corpus() + list(corpus.ref_inputs(ref_tests).values())
    compared = 0
    for inst in insts:
        base = corpus.reference(inst, 1.0)
        assert base["status"] == 0
        cbs = cbs_ta_corpus.reference(inst)
        if cbs["status"] == 0:
            assert base["cost"] == cbs["cost"], (inst, base["cost"], cbs["cost"])
            compared += 1
        else:
            assert base["reached"]["first_assignment_empty"] == 1 and base["cost"] == 0
        for w in corpus.WS:
            r = corpus.reference(inst, w)
            assert r["status"] == 0 and r["cost"] <= w * base["cost"], (inst, w, r["cost"], base["cost"])
            assert _first_conflict(r["paths_xy"]) is None
            assert [p[-1] for p in r["paths_xy"]] == [e[:2] for e in r["ends"]]
    assert compared >= 40


def test_the_corpus_reaches_what_it_is_for():
    """Counted over the (instance, w) pairs: at least a third expand a node with a conflict, at least five push a second root,
    at least one has a child search that fails, and at least one instance has an empty FIRST assignment.
    The condition "a root that fails part-way" is dropped, because no input can meet it: a root's searches carry no
    constraints; an agent without a task ends at its start, and an agent is only ever assigned a goal that its shortest-path
    table reaches from its start (an unreachable pair is no edge of the assignment problem), so every root search finds a
    path.  A root ends early only under an expansion budget, which ends the instance instead (test_ecbs_ta_driver_cpu.py)."""
    assert 40 <= len(corpus.SEEDS) <= 60
    refs = [corpus.reference(i, w) for i, w in corpus.pairs()]
    assert all(r["status"] == 0 for r in refs)
    assert sum(1 for r in refs if r["reached"]["conflict_nodes"] > 0) * 3 >= len(refs)
    assert sum(1 for r in refs if r["n_roots"] >= 2) >= 5
    assert sum(1 for r in refs if r["reached"]["child_failures"] > 0) >= 1
    assert sum(1 for i in corpus.corpus() if corpus.reference(i, 1.0)["reached"]["first_assignment_empty"]) >= 1
    assert all(r["reached"]["roots_failed_part_way"] == 0 for r in refs)
    assert len({r["cost"] for r in (corpus.reference(corpus.instance(277), w) for w in corpus.WS)}) > 1  # w changes an answer
    assert any(len({tuple(g) for gs in i["potential_goals"] for g in gs}) < len(i["starts"]) for i in corpus.corpus())
