"""MRP_LL_JOB_TRY_LDS in the host packer (csrc/host/ll_pack.h packJob) as a stand-alone program under the host sanitizers:
the flag reaches ctx_flags of an MRP_LL_ASTAR_EPS_TA job and changes nothing else, combines with MRP_LL_JOB_NO_GOAL,
MRP_LL_JOB_STORE_RESULT and path_ids, is dropped for the other algorithms, is never set by a zero-initialised job, and
what is rejected stays rejected (tests/support/eps_ta_try_lds_pack_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_try_lds_in_the_packer():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "eps_ta_try_lds_pack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + ["-o", exe, os.path.join(SUPPORT, "eps_ta_try_lds_pack_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "eps_ta_try_lds_pack_check: ok" in run.stdout
