"""hl.solve_ecbs_ta_batch under MRP_HL_TA_DEVICE_PATHS=1 on the MI355X: every path stays in the engine's path store, roots
through mrp_ll_ta_eps_root_batch_stored or as jobs that store their results, child contexts by slot — against the sequential
restatement (tests/ecbs_ta_tree_corpus.py) at every w of the corpus, plus the reference's three inputs, with both root forms;
and once more with a store so small that the free list runs dry and most contexts are shipped."""
import pytest

import ecbs_ta_tree_corpus as corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def insts(ref_tests, oracle_mod):
    return corpus.corpus() + list(corpus.ref_inputs(ref_tests).values())


def _check(got, stats, insts, w):
    for g, i in zip(got, insts):
        corpus.same(g, corpus.reference(i, w))
    if w == 1.0:
        assert [g["cost"] for g in got[-3:]] == [6, 6, 5]
    assert stats["solved"] == len(insts)


@pytest.mark.parametrize("use_root_kernel", [0, 1])
@pytest.mark.parametrize("w", corpus.WS)
def test_device_paths_equal_the_restatement(insts, monkeypatch, w, use_root_kernel):
    from libmultirobotplanning_amd import hl
    monkeypatch.setenv("MRP_HL_TA_DEVICE_PATHS", "1")
    got, stats = hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=bool(use_root_kernel))
    _check(got, stats, insts, w)


@pytest.mark.parametrize("use_root_kernel", [0, 1])
def test_a_store_that_runs_dry_gives_the_same_answers(insts, monkeypatch, use_root_kernel):
    """60 slots for a corpus whose roots alone need more (tests/test_ecbs_ta_store_driver_cpu.py shows both forms of job in the
    stand-in's log at this size)."""
    from libmultirobotplanning_amd import hl
    monkeypatch.setenv("MRP_HL_TA_DEVICE_PATHS", "1")
    monkeypatch.setenv("MRP_HL_TA_PATH_SLOTS", "60")
    got, stats = hl.solve_ecbs_ta_batch(insts, 1.3, use_root_kernel=bool(use_root_kernel))
    _check(got, stats, insts, 1.3)
