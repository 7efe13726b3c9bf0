"""The path-store form of MRP_LL_ASTAR_EPS_TA in the host packers (csrc/host/ll_pack.h packJob, ta_eps_root_pack.h) as a
stand-alone program under the host sanitizers: the descriptor of a job that names its context by path-store slots and
stores its result, the jobs the packer refuses with nothing pushed, and the root packer with and without slot ids
(tests/support/eps_ta_store_pack_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_eps_ta_store_packers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "eps_ta_store_pack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + ["-o", exe, os.path.join(SUPPORT, "eps_ta_store_pack_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "eps_ta_store_pack_check: ok" in run.stdout
