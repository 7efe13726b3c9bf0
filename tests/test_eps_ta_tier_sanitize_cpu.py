"""The LDS tier of MRP_LL_ASTAR_EPS_TA (csrc/ll_compact_ta_eps.h) on the emulator as a stand-alone program under the host
sanitizers (tests/support/ta_eps_sanitize_main.cpp): 600 seeded searches with every kind of exit; the sanitizers watch the
tier's accesses to what stands for device memory — cameFrom table, focal path table, heuristic table, constraint words, the
path out —, the emulator those to its window."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_seeded_searches_under_the_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "ta_eps_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall"] + SAN +
                          ["-o", exe, os.path.join(SUPPORT, "ta_eps_sanitize_main.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert run.returncode == 0, run.stdout
    assert "ta_eps_sanitize: 600 searches, 0 wrong" in run.stdout
