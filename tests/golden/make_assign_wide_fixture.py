"""Writes tests/golden/assign_wide_task_of.json: the results — task_of included — of the wide assignment wave program on
the CPU emulator (tests/support/emu_assign_wide.cpp) for the shapes and the constraints beyond bit 63 of
tests/assignment_wide_inputs.py.  Both row sources must agree before anything is written.  The CPU and the GPU test
compare against this one file.
usage: python tests/golden/make_assign_wide_fixture.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import assignment_wide_inputs as wi  # noqa: E402
import test_assign_wide_emu_cpu as emu_test  # noqa: E402

run = emu_test.build_emu()
probs = dict(wi.shape_problems())
probs.update({n: p for n, (p, _) in wi.constraint_problems().items()})
names = wi.recorded_names()
res = [emu_test.solve_all(run, [probs[n] for n in names], b) for b in emu_test.BUDGETS]
assert res[0] == res[1], "the two row sources disagree"
with open(wi.GOLDEN_FILE, "w") as f:
    json.dump({n: [r[0], r[1], r[2], r[3]] for n, r in zip(names, res[0])}, f, separators=(",", ":"))
    f.write("\n")
print("wrote", len(names), "results")
