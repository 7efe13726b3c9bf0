"""hl.solve_ecbs_ta_batch on the MI355X: the batched ECBS-TA driver over the real engine — tables, next-best series, root
kernel and MRP_LL_ASTAR_EPS_TA searches on the device — against the sequential restatement (tests/ecbs_ta_tree_corpus.py) at
every w of the corpus, plus the reference's three inputs, with roots as one call and as dependent jobs."""
import pytest

import ecbs_ta_tree_corpus as corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def insts(ref_tests, oracle_mod):
    return corpus.corpus() + list(corpus.ref_inputs(ref_tests).values())


@pytest.mark.parametrize("use_root_kernel", [0, 1])
@pytest.mark.parametrize("w", corpus.WS)
def test_one_batch_equals_the_restatement(insts, w, use_root_kernel):
    from libmultirobotplanning_amd import hl
    got, stats = hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=bool(use_root_kernel))
    for g, i in zip(got, insts):
        corpus.same(g, corpus.reference(i, w))
    if w == 1.0:
        assert [g["cost"] for g in got[-3:]] == [6, 6, 5]
    assert stats["solved"] == len(insts)


def test_one_instance_and_an_empty_batch(insts):
    from libmultirobotplanning_amd import hl
    w = 1.3
    deep = max(range(len(insts)), key=lambda q: corpus.reference(insts[q], w)["hl_expanded"])
    for k in (True, False):
        got, _ = hl.solve_ecbs_ta_batch([insts[deep]], w, use_root_kernel=k)
        corpus.same(got[0], corpus.reference(insts[deep], w))
    got, stats = hl.solve_ecbs_ta_batch([], w)
    assert got == [] and stats["rounds"] == 0
