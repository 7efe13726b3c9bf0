"""The wide assignment packer (libmultirobotplanning_amd/csrc/host/assign_pack.h: packAssignBatchWide) and the next-best
series generalised to mask words (host/assign_series.h), both pure host logic, under the host sanitizers:
tests/support/assign_wide_host_check.cpp is a program of its own that checks the limits (257, mask_words 0 and 5, a
mask_words too small for n_tasks), the staged words of a 65 x 130 problem, the row-source choice at the budget's edge,
that a narrow series built through the generalised code stages the words it staged before, and a narrow and a wide series
advancing in one step with one solver call each.  The sanitizers are linked in the ordinary way; the program exits
non-zero at its first failed check or sanitizer report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_packer_and_series_under_host_sanitizers():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "assign_wide_host_check")
    csrc = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc")
    sup = os.path.join(ROOT, "tests", "support")
    deps = [os.path.join(sup, "assign_wide_host_check.cpp"), os.path.join(sup, "wave_emu_assign.h"), os.path.join(sup, "wave_emu.h"),
            os.path.join(csrc, "host", "assign_pack.h"), os.path.join(csrc, "host", "assign_series.h"),
            os.path.join(csrc, "host", "ll_pack.h"), os.path.join(csrc, "assign_layout.h"), os.path.join(csrc, "assign_wave.h"),
            os.path.join(csrc, "assign_wave_wide.h"), os.path.join(csrc, "heur_layout.h"), os.path.join(ROOT, "include", "mrp_ll.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, deps[0]])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "assign_wide_host_check: ok" in run.stdout
