"""The assignment packer (libmultirobotplanning_amd/csrc/host/assign_pack.h: pure host logic, no HIP) under the host
sanitizers: tests/support/assign_host_check.cpp is a program of its own that checks validation only — a dimension, a cost,
a forced task, a required cardinality, a heuristic id or a start out of range gives MRP_LL_BAD_JOB for that problem, and
its neighbours are staged exactly as without it.  The sanitizers are linked in the ordinary way; the program exits
non-zero at its first failed check or sanitizer report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assignment_packer_validation_under_host_sanitizers():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "assign_host_check")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [os.path.join(ROOT, "tests", "support", "assign_host_check.cpp"), os.path.join(csrc, "host", "assign_pack.h"),
            os.path.join(csrc, "host", "ll_pack.h"), os.path.join(csrc, "assign_layout.h"), os.path.join(csrc, "heur_layout.h"),
            os.path.join(ROOT, "include", "mrp_ll.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, deps[0]])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "assign_host_check: ok" in run.stdout
