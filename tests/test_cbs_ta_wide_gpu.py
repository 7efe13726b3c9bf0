"""hl.solve_cbs_ta_batch beyond 64 agents on the MI355X: the batched CBS-TA driver over the real engine — wide next-best
series, wide root kernel, task-assignment searches — against the wide restatement (tests/ta_wide_corpus.py) with roots as
one call and as ordinary jobs, an independent validator on every solved answer, a batch that mixes narrow and wide instances,
and one run of the cbs_ta command-line tool on a 65-agent input."""
import yaml

import pytest

import cbs_ta_corpus as narrow
import ta_wide_corpus as wide

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def refs(oracle_mod):
    return wide.references()


@pytest.mark.parametrize("use_root_kernel", [0, 1])
def test_wide_corpus_equals_the_wide_restatement(refs, use_root_kernel):
    from libmultirobotplanning_amd import hl
    named = wide.named()
    free = [n for n, (_, cap) in named.items() if cap < 0]
    got, stats = hl.solve_cbs_ta_batch([named[n][0] for n in free], use_root_kernel=bool(use_root_kernel), path_cap=128)
    for n, g in zip(free, got):
        wide.same(g, refs[n])
        assert g["status"] == hl.SOLVED
        wide.validate(named[n][0], g)
    assert stats["solved"] == len(free)
    caps = [n for n, (_, cap) in named.items() if cap >= 0]
    capped, _ = hl.solve_cbs_ta_batch([named[n][0] for n in caps], use_root_kernel=bool(use_root_kernel), max_hl_expansions=wide.CAP_HL,
                                      path_cap=128)
    for n, g in zip(caps, capped):
        wide.same(g, refs[n])
        assert g["status"] == hl.CAP and g["hl_expanded"] == wide.CAP_HL


@pytest.mark.parametrize("use_root_kernel", [0, 1])
def test_mixed_batch(refs, use_root_kernel):
    from libmultirobotplanning_amd import hl
    small = narrow.corpus()[:8]
    names = ["a65", "cross", "a81", "cross_back"]
    insts, want = [], []
    for q in range(8):
        insts.append(small[q])
        want.append(narrow.reference(small[q]))
        if q < len(names):
            insts.append(wide.named()[names[q]][0])
            want.append(refs[names[q]])
    got, _ = hl.solve_cbs_ta_batch(insts, use_root_kernel=bool(use_root_kernel), path_cap=128)
    for g, r in zip(got, want):
        wide.same(g, r)


def test_cbs_ta_cli_on_a_65_agent_input(tmp_path, refs):
    from libmultirobotplanning_amd import cli
    inst = wide.named()["a65"][0]
    doc = {"map": {"dimensions": [inst["dimx"], inst["dimy"]], "obstacles": inst["obstacles"]},
           "agents": [{"name": "agent%d" % i, "start": s, "potentialGoals": g}
                      for i, (s, g) in enumerate(zip(inst["starts"], inst["potential_goals"]))]}
    with open(tmp_path / "in.yaml", "w") as f:
        yaml.safe_dump(doc, f)
    assert cli.main(["cbs_ta", "-i", str(tmp_path / "in.yaml"), "-o", str(tmp_path / "out.yaml")]) == 0
    out = yaml.safe_load(open(tmp_path / "out.yaml"))
    ref = refs["a65"]
    st = out["statistics"]
    assert (st["cost"], st["highLevelExpanded"], st["numTaskAssignments"]) == (ref["cost"], ref["hl_expanded"], ref["num_task_assignments"])
    assert len(out["schedule"]) == 65
    for a, end in enumerate(ref["ends"]):
        last = out["schedule"]["agent%d" % a][-1]
        assert [last["x"], last["y"], last["t"]] == end
