"""The wide restatements of CBS-TA and ECBS-TA (tests/support/cbs_ta_tree_wide_check.cpp, ecbs_ta_tree_wide_check.cpp: masks of
mask_words words, the series over the WIDE assignment wave program on the CPU) pinned to the existing ones: on every instance
of cbs_ta_corpus.corpus(), of ecbs_ta_tree_corpus (at every w) and on the reference's three mapfta_* inputs they return field
for field what cbs_ta_tree_check.cpp / ecbs_ta_tree_check.cpp return; and the wide corpus meets the conditions its seeds
were chosen for."""
import time

import cbs_ta_corpus as narrow
import ecbs_ta_tree_corpus as narrow_ecbs
import ta_wide_corpus as wide


def test_wide_ecbs_restatement_equals_the_narrow_one_on_the_narrow_corpus(ref_tests):
    named = narrow_ecbs.ref_inputs(ref_tests)
    insts = narrow_ecbs.corpus() + list(named.values())
    for w in narrow_ecbs.WS:
        for inst in insts:
            assert wide.reference_ecbs(inst, w) == narrow_ecbs.reference(inst, w)
        for max_ta, max_hl in ((0, -1), (1, -1), (2 ** 30, 2)):
            for inst in insts[::5]:
                assert wide.reference_ecbs(inst, w, max_ta, max_hl) == narrow_ecbs.reference(inst, w, max_ta, max_hl)
    assert [wide.reference_ecbs(i, 1.0)["cost"] for i in named.values()] == [6, 6, 5]


def test_wide_restatement_equals_the_narrow_one_on_the_narrow_corpus(ref_tests):
    named = narrow.ref_inputs(ref_tests)
    insts = narrow.corpus() + list(named.values())
    for inst in insts:
        assert wide.reference(inst) == narrow.reference(inst)
    for max_ta, max_hl in ((0, -1), (1, -1), (2 ** 30, 2)):
        for inst in insts[::5]:
            assert wide.reference(inst, max_ta, max_hl) == narrow.reference(inst, max_ta, max_hl)
    assert [wide.reference(i)["cost"] for i in named.values()] == [6, 6, 5]


def test_the_wide_corpus_is_what_it_is_for():
    t0 = time.time()
    refs = wide.references()
    took = time.time() - t0
    insts = wide.named()
    assert sorted(len(i["starts"]) for i, _ in insts.values()) == [65, 66, 70, 72, 72, 80, 81, 96, 128, 129, 256]
    tasks = {n: len({tuple(g) for gs in i["potential_goals"] for g in gs}) for n, (i, _) in insts.items()}
    assert tasks["a129"] > 128 and tasks["fewer_tasks"] < 70 and tasks["more_tasks"] > 66 and tasks["cross"] > 64
    cross = insts["cross"][0]["potential_goals"]
    order = []
    for gs in cross:
        order.extend(tuple(g) for g in gs if tuple(g) not in order)
    assert all(order.index(tuple(g)) < 64 for gs in cross[64:] for g in gs)  # agents from 64 on: tasks below 64 only
    assert any(all(tuple(g) not in map(tuple, gs) for gs in cross[64:]) for g in order[64:])  # a task >= 64 for agents < 64 only
    back = insts["cross_back"][0]["potential_goals"]
    order = []
    for gs in back:
        order.extend(tuple(g) for g in gs if tuple(g) not in order)
    first_new = len({tuple(g) for gs in back[:64] for g in gs})
    assert first_new < min(64, len(order))  # task first_new: below 64, allowed to agents from 64 on only
    assert all(order.index(tuple(g)) >= first_new for gs in back[64:] for g in gs)
    for name in [n for n, (_, cap) in insts.items() if cap >= 0]:
        capped = refs.pop(name)
        assert capped["status"] == 2 and capped["hl_expanded"] == wide.CAP_HL
    assert all(r["status"] == 0 and r["hl_expanded"] <= 100 for r in refs.values())
    assert 3 * sum(1 for r in refs.values() if r["root_conflicts"] >= 1) >= len(refs)
    assert sum(1 for r in refs.values() if r["n_roots"] >= 3) >= 3
    idle = refs["fewer_tasks"]["tasks"].count(None)
    assert idle >= 70 - tasks["fewer_tasks"] > 0
    assert took < 60
