"""hl.solve_ecbs_ta_batch beyond 64 agents on the MI355X: the batched ECBS-TA driver over the real engine — wide next-best
series, wide ECBS-TA root kernel, focal task-assignment searches — against the wide restatement
(tests/support/ecbs_ta_tree_wide_check.cpp through tests/ta_wide_corpus.py) field for field, at w = 1.0 and 1.3, with roots
as one call and as dependent jobs; the independent validator on every solved answer; a batch that mixes narrow and wide
instances, also under MRP_HL_TA_DEVICE_PATHS=1."""
import pytest

import ecbs_ta_tree_corpus as narrow
import ta_wide_corpus as wide

pytestmark = pytest.mark.gpu

WS = (1.0, 1.3)
MIXED = ("a65", "cross", "a81", "cross_back")


@pytest.mark.parametrize("use_root_kernel", [0, 1])
@pytest.mark.parametrize("w", WS)
def test_wide_corpus_equals_the_wide_restatement(oracle_mod, w, use_root_kernel):
    from libmultirobotplanning_amd import hl
    named = wide.ecbs_named(w)
    solved = 0
    for cap in sorted({c for _, c in named.values()}):
        names = [n for n, (_, c) in named.items() if c == cap]
        got, _ = hl.solve_ecbs_ta_batch([named[n][0] for n in names], w, use_root_kernel=bool(use_root_kernel), max_hl_expansions=cap,
                                        path_cap=128)
        for n, g in zip(names, got):
            narrow.same(g, wide.reference_ecbs(named[n][0], w, max_hl=cap))
            if g["status"] == hl.SOLVED:
                wide.validate(named[n][0], g)
                solved += 1
            elif cap >= 0:
                assert g["status"] == hl.CAP and g["hl_expanded"] == cap
    assert solved >= (len(named) - 1 if w > 1.0 else len(named) - 3)  # all but the capped ones (w > 1: only the 256-agent one)


@pytest.mark.parametrize("device_paths", ["0", "1"])
@pytest.mark.parametrize("w", WS)
def test_mixed_batch(oracle_mod, monkeypatch, w, device_paths):
    from libmultirobotplanning_amd import hl
    monkeypatch.setenv("MRP_HL_TA_DEVICE_PATHS", device_paths)
    small = narrow.corpus()[:8]
    insts, want = [], []
    for q in range(8):
        insts.append(small[q])
        want.append(narrow.reference(small[q], w))
        if q < len(MIXED):
            insts.append(wide.named()[MIXED[q]][0])
            want.append(wide.reference_ecbs(insts[-1], w))
    for use_root_kernel in (False, True):
        got, _ = hl.solve_ecbs_ta_batch(insts, w, use_root_kernel=use_root_kernel, path_cap=128)
        for g, r in zip(got, want):
            narrow.same(g, r)
