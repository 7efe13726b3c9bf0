"""The arena slot's layout (libmultirobotplanning_amd/csrc/ll_slot.h: sizes and scratch areas, shared by mrp_ll_create and
the device searches) under the host sanitizers: tests/support/slot_layout_check.cpp is a program of its own that compiles
the header with g++ alone and checks it over arena_nodes {131072, 4096, 2} x max_horizon {512, 1, 1024} x max_cells
{4096, 1, 65025} — areas in order and disjoint inside a heap block of exactly the stride, 256-byte multiples, the numbers of
the formula mrp_ll_create used to write out, three of them worked by hand.  The sanitizers are linked in the ordinary way;
the program exits non-zero at its first failed check or sanitizer report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_layout_under_host_sanitizers():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "slot_layout_check")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    deps = [os.path.join(ROOT, "tests", "support", "slot_layout_check.cpp"), os.path.join(csrc, "ll_slot.h"),
            os.path.join(csrc, "ll_device.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, deps[0]])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "slot_layout_check: ok" in run.stdout
