"""The host packers of mrp_ll_ta_root_batch_w / mrp_ll_ta_eps_root_batch_w (csrc/host/ta_root_pack.h, ta_eps_root_pack.h with
the agent limit as a parameter) as stand-alone programs under the host sanitizers: tests/support/ta_root_wide_pack_check.cpp,
once plain and once with -DEPS.  And the two new symbols are exported by the engine library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = os.path.join(ROOT, "tests", "support")
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("eps", [False, True])
def test_wide_root_packers(eps):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "ta_root_wide_pack_check" + ("_eps" if eps else ""))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + (["-DEPS"] if eps else []) +
                          ["-o", exe, os.path.join(SUPPORT, "ta_root_wide_pack_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-2000:]


def test_wide_root_calls_are_exported():
    from libmultirobotplanning_amd import _build, ll
    _build.build()
    lib = ll.load_library()
    for name in ("mrp_ll_ta_root_batch_w", "mrp_ll_ta_eps_root_batch_w"):
        assert hasattr(lib, name) and name in ll.EXPORTS
