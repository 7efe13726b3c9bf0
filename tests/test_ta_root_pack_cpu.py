"""The packer and unpacker of mrp_ll_ta_root_batch (csrc/host/ta_root_pack.h) as a stand-alone program under the host
sanitizers: refusals, the 64-agent record, the word offsets, the per-agent descriptor against packJob's for the ordinary
job, a root that ended behind an agent, a scan left to the host (tests/support/ta_root_pack_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_root_packer_and_unpacker():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "ta_root_pack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + ["-o", exe, os.path.join(SUPPORT, "ta_root_pack_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "ta_root_pack_check: ok" in run.stdout
