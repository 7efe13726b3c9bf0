"""The packer and unpacker of mrp_ll_ta_eps_root_batch (csrc/host/ta_eps_root_pack.h) as a stand-alone program under the
host sanitizers: the root's record with its weight, the per-agent descriptor against packJob's for the ordinary
MRP_LL_ASTAR_EPS_TA job that ships the paths before it, and the way back — a root left unfinished because its table did not
fit, a scan left to the host, a root that ended behind an agent (tests/support/ta_eps_root_pack_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_eps_root_packer_and_unpacker():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "ta_eps_root_pack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + ["-o", exe, os.path.join(SUPPORT, "ta_eps_root_pack_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "ta_eps_root_pack_check: ok" in run.stdout
