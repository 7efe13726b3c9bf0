"""The CBS-TA and ECBS-TA drivers (csrc/hl/mrp_hl_ta.cpp, csrc/hl/mrp_hl_ecbs_ta.cpp over csrc/hl/ta_rounds.hpp) on the stand-in
engines as a stand-alone program under the host sanitizers (tests/support/ta_driver_sanitize_main.cpp): a batch of seeded small
instances, two without a reachable goal and one of 65 agents through both entry points with roots as one call and as jobs,
ECBS-TA also under MRP_HL_TA_DEVICE_PATHS=1 with eight slots; the sanitizers watch the result, root and job records'
pointers into the round's buffers and the paths' slot hand-backs.  Linked as test_ecbs_ta_wide_driver_cpu.py's store_driver."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
HL = os.path.join(ROOT, "libmultirobotplanning_amd", "csrc", "hl")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_both_drivers_under_the_sanitizers(oracle_mod):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "ta_driver_sanitize")
    srcs = [os.path.join(SUPPORT, "ta_driver_sanitize_main.cpp")] + \
           [os.path.join(HL, f) for f in ("mrp_hl.cpp", "mrp_hl_ta.cpp", "mrp_hl_ecbs_ta.cpp")] + \
           [os.path.join(SUPPORT, f) for f in ("mock_ll_ta_eps_wide.cpp", "mock_ll_ta_assign.cpp", "mock_ll_ta_assign_wide.cpp",
                                               "ecbs_ta_check.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread"] + SAN + ["-DMOCK_TA_WIDE_BASE=\"mock_ll_ta_eps_store.cpp\"",
                          "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), "-I", SUPPORT, "-o", exe] + srcs +
                          ["-Wl,--wrap=mrp_ll_search_batch", "-L", os.path.join(ROOT, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRP_")}
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout
    assert "ta_driver_sanitize: 0 wrong" in run.stdout
    assert run.stdout.count("15 instances") == 10  # CBS-TA twice, ECBS-TA four times at each of two weights
