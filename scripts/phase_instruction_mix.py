#!/usr/bin/env python3
"""Static instruction mix of the phases of compactSearch's expansion loop (csrc/ll_compact.h), from the assembly alone.

Compiles ll_kernel.hip for gfx950, device only, with -DMRP_CT_ASM_MARKS ("; PHASE k" comments at the phase boundaries, the
marks of the -DMRP_CT_PROF build) and counts, for the narrow and the wide instance that keep bitmap and focal table in device
memory (EPS, !PLDS, BG: what the front and the heavy workgroups run), the instructions that stand between each mark and the
next one in the text of the function — static counts, one pass, every instruction once (a loop counts one turn, both sides of a
branch count).  The compiler lays the loop out in source order, so "2 .. 3" is pop + erase, "3 .. 4" the successors' entries
and "4 .. 5" the pushes; the other lines (0: set-up, loop top and probes, 1: behind a walk, the last one: everything up to the
function's end) hold whatever blocks the layout put there and are printed for completeness.

Columns: SALU (s_* but branches and waits), branch (s_branch, s_cbranch*), VALU (v_* but the lane operations), lane
(v_readlane, v_writelane, v_readfirstlane), LDS (ds_*), vmem (global_ / buffer_ / flat_ / scratch_), wait (s_waitcnt).
Below the table: registers and scratch of the function as the compiler reports them.

No GPU needed.  usage: python scripts/phase_instruction_mix.py [--root DIR] [--define MACRO ...] >> profiles/<tag>_phase_instruction_mix.txt"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_wait_placement as pw  # noqa: E402

KINDS = ("SALU", "branch", "VALU", "lane", "LDS", "vmem", "wait")
LANE = ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32")
RES = re.compile(r"^; (NumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|SGPRBlocks|VGPRBlocks):\s*(\S+)|^;\s+(sgpr_spill_count|vgpr_spill_count):\s*(\S+)")


def kind(op):
    if op == "s_waitcnt":
        return "wait"
    if op == "s_branch" or op.startswith("s_cbranch"):
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    if op in LANE:
        return "lane"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(pw.VMEM):
        return "vmem"
    return None


def analyse(lines):
    """{instance tuple: ([(mark, next mark or None, Counter of kinds)] in text order, {resource: value})} for the EPS, !PLDS,
    BG instances."""
    res = {}
    for name, inst, lo, hi in pw.instances(lines):
        if not (inst[0] and not inst[1] and inst[2]):
            continue
        f = pw.Func(lines, lo, hi)
        marks = [(i, f.mark(i)) for i in range(lo, hi) if f.mark(i) is not None]
        spans = []
        for n, (i, k) in enumerate(marks):
            end, nxt = (marks[n + 1][0], marks[n + 1][1]) if n + 1 < len(marks) else (hi, None)
            spans.append((k, nxt, collections.Counter(kind(f.insn(j)[0]) for j in range(i, end) if f.insn(j))))
        regs = {}
        for i in range(hi, min(hi + 60, len(lines))):
            m = RES.match(lines[i])
            if m:
                regs[m.group(1) or m.group(3)] = m.group(2) or m.group(4)
        res[inst] = (spans, regs)
    return res


def report(res, tag):
    out = ["== %s" % tag]
    for inst in sorted(res):
        mix, regs = res[inst]
        out.append(pw.label_of(inst))
        out.append("  marks       | " + " | ".join("%6s" % k for k in KINDS) + " | SALU + branch")
        for k, nxt, c in mix:
            out.append("  %4d .. %-4s | " % (k, "end" if nxt is None else nxt) + " | ".join("%6d" % c.get(q, 0) for q in KINDS) + " | %d" % (c.get("SALU", 0) + c.get("branch", 0)))
        out.append("  " + "  ".join("%s %s" % kv for kv in sorted(regs.items())))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--define", action="append", default=[],
                    help="a further -D macro: MRP_CT_PLAIN_EXPANSION, MRP_CT_SCALAR_PUSHES, MRP_CT_LOAD_TOPS, MRP_CT_KEEP_TOPS ...")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="phase_mix_")
    try:
        out = os.path.join(tmp, "marks.s")
        src = os.path.join(a.root, "libmultirobotplanning_amd", "csrc")
        cmd = [pw.HIPCC] + pw.FLAGS + ["-I", os.path.join(a.root, "include"), "-DMRP_CT_ASM_MARKS"] + ["-D" + d for d in a.define] + \
              ["ll_kernel.hip", "-o", out]
        p = subprocess.run(cmd, cwd=src, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if p.returncode != 0:
            raise RuntimeError("hipcc failed (exit %d):\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-3000:]))
        lines = open(out).read().split("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(report(analyse(lines), a.tag + (" (" + " ".join("-D" + d for d in a.define) + ")" if a.define else "")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
