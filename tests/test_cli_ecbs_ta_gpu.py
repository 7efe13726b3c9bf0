"""The ecbs_ta front-end (example/ecbs_ta.cpp:587-695 schema) end to end on the GPU, on the reference's own test input:
test/test_ecbs_ta.py at w = 1.0 — cost 6, agent0 ends at x 4, y 0, t 4, agent1 at (2, 1)."""
import yaml

import pytest

pytestmark = pytest.mark.gpu


def test_ecbs_ta_cli_on_the_reference_input(tmp_path, ref_tests):
    from libmultirobotplanning_amd import cli
    inst = ref_tests["cbs_ta"]["inputs"]["mapfta_simple1_a2"]
    doc = {"map": {"dimensions": [inst["dimx"], inst["dimy"]], "obstacles": inst["obstacles"]},
           "agents": [{"name": "agent%d" % i, "start": s, "potentialGoals": g}
                      for i, (s, g) in enumerate(zip(inst["starts"], inst["potential_goals"]))]}
    with open(tmp_path / "in.yaml", "w") as f:
        yaml.safe_dump(doc, f)
    assert cli.main(["ecbs_ta", "-i", str(tmp_path / "in.yaml"), "-o", str(tmp_path / "out.yaml"), "-w", "1.0",
                     "--maxTaskAssignments", "100"]) == 0
    out = yaml.safe_load(open(tmp_path / "out.yaml"))
    st = out["statistics"]
    assert st["cost"] == 6
    assert list(st.keys()) == ["cost", "makespan", "runtime", "highLevelExpanded", "lowLevelExpanded", "numTaskAssignments"]
    assert st["numTaskAssignments"] >= 1
    assert out["schedule"]["agent0"][-1] == {"x": 4, "y": 0, "t": 4}
    last = out["schedule"]["agent1"][-1]
    assert (last["x"], last["y"]) == (2, 1)
