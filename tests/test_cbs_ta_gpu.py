"""hl.solve_cbs_ta_batch on the MI355X: the batched CBS-TA driver over the real engine — tables, next-best series, root
kernel and task-assignment searches on the device — against the sequential restatement (tests/cbs_ta_corpus.py), with roots
as one call and as ordinary jobs."""
import pytest

import cbs_ta_corpus as corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected(ref_tests, oracle_mod):
    named = corpus.ref_inputs(ref_tests)
    insts = corpus.corpus() + list(named.values())
    return insts, [corpus.reference(i) for i in insts]


@pytest.mark.parametrize("use_root_kernel", [0, 1])
def test_one_batch_equals_the_restatement(expected, use_root_kernel):
    from libmultirobotplanning_amd import hl
    insts, refs = expected
    got, stats = hl.solve_cbs_ta_batch(insts, use_root_kernel=bool(use_root_kernel))
    for g, r in zip(got, refs):
        corpus.same(g, r)
    assert [g["cost"] for g in got[-3:]] == [6, 6, 5]
    assert stats["solved"] == len(insts)


def test_one_instance_and_an_empty_batch(expected):
    from libmultirobotplanning_amd import hl
    insts, refs = expected
    deep = max(range(len(insts)), key=lambda q: refs[q]["hl_expanded"])
    got, _ = hl.solve_cbs_ta_batch([insts[deep]], use_root_kernel=True)
    corpus.same(got[0], refs[deep])
    got, stats = hl.solve_cbs_ta_batch([])
    assert got == [] and stats["rounds"] == 0
