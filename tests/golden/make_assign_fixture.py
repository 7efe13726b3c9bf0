"""Writes tests/golden/assign_task_of.json: the results — task_of included — of the assignment wave program on the CPU
emulator (tests/support/emu_assign.cpp) for the problem sets of tests/assignment_inputs.py recorded_sets().  The CPU and
the GPU test compare against this one file: that is how "the emulator and the device give the same task_of" is held.
usage: python tests/golden/make_assign_fixture.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import assignment_inputs as ai  # noqa: E402
import test_assign_emu_cpu as emu_test  # noqa: E402

run = emu_test.build_emu()
out = {name: [[r[0], r[1], r[2], r[3]] for r in emu_test.solve_all(run, problems)]
       for name, problems in ai.recorded_sets().items()}
with open(os.path.join(HERE, "assign_task_of.json"), "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
print("wrote", sum(len(v) for v in out.values()), "results")
