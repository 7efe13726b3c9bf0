"""Where the compiler waits for the focal-table row loads (scripts/probe_wait_placement.py; no GPU: ll_kernel.hip is compiled
device-only to assembly with -DMRP_CT_ASM_MARKS, about half a minute).

The searches that read the focal path table from device memory issue the loads of rows t and t + 1 in front of the pops of
an expansion so that the round trip hides behind the pops.  That holds only while nothing between the loads and the pop uses
a loaded value: a select on the value puts an s_waitcnt vmcnt(0) in front of the pop (and makes every load an exec region).
In the two instances the front and the heavy workgroups run (BG, narrow and wide) no s_waitcnt vmcnt at all may stand between
a row load and the PHASE 2 mark, on any path: all four loads are in flight at the pop.  With the loaded values selected at the
load (`sel(in0, gLoadU16m(...), 0xFFFF)`) the tool reports "4 waited before the pop" in all three instances.

The third instance (EPS, table in memory, bitmap in LDS; not on the headline's path) is reported, and held to the weaker
property that matters: no wait for one of THIS expansion's loads.  It keeps two waits that are followed by loads, vmcnt(1)
and vmcnt(2): they guard the registers of the previous expansion's loads for rows of more than 64 agents, which nothing has
read when that expansion had no valid successor (`continue`), against being overwritten; the counts leave this expansion's
loads in flight, and the loads they do wait for were issued a whole pop earlier."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import probe_wait_placement as pw  # noqa: E402

NARROW_BG, WIDE_BG, NARROW_LDS_BITMAP = (True, False, True, False), (True, False, True, True), (True, False, False, False)


@pytest.fixture(scope="module")
def marks():
    (asm,) = pw.build_and_read(ROOT, marks_only=True)
    res = pw.analyse_marks(asm)
    print(pw.report(res))
    return res


def test_the_three_instances_are_found(marks):
    assert set(marks) == {NARROW_BG, WIDE_BG, NARROW_LDS_BITMAP}
    for r in marks.values():
        assert r["loads"] == 4  # rows t and t + 1, columns 0 .. 63 and 64 .. 127


@pytest.mark.parametrize("inst", [NARROW_BG, WIDE_BG], ids=["narrow", "wide"])
def test_no_wait_between_the_row_loads_and_the_pop(marks, inst):
    r = marks[inst]
    assert (r["followed"], r["waited"], r["in_flight"]) == (0, 0, 4), r


def test_the_third_instance_waits_for_none_of_its_own_loads(marks):
    r = marks[NARROW_LDS_BITMAP]
    print("compactSearch<true, false, false>: %d of 4 row loads followed by some s_waitcnt vmcnt, %d waited before the pop" %
          (r["followed"], r["waited"]))
    assert (r["waited"], r["in_flight"]) == (0, 4), r
