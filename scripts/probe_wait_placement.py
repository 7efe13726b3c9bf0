#!/usr/bin/env python3
"""Where the compiler waits for the focal-table row loads of compactSearch (csrc/ll_compact.h), from the assembly alone.

The instances that read the focal path table from device memory (EPS, !PLDS) issue the loads of the table's rows t and t + 1
in front of the pops of an expansion; the loads are worth issuing there only if nothing waits for them before the pops are
done.  This tool compiles ll_kernel.hip for gfx950, device only, twice:

  * with -DMRP_CT_ASM_MARKS ("; PHASE k" comments at the phase boundaries): for every global_load_ushort between a
    PHASE 0 mark (the probes) and the next PHASE 2 mark (the pop) it walks every path of the function's control flow from
    the load to the PHASE 2 mark and records the s_waitcnt vmcnt(N) it meets — any of them ("followed by a wait") and those
    that wait for this very load (fewer than N + 1 vector-memory instructions issued behind it: "waited before the pop");
  * as the product is built: for every global_load_ushort of those instances, the fewest instructions on any path between
    the load and the first s_waitcnt that waits for it, and how many of them are LDS instructions.

No GPU needed.  usage: python scripts/probe_wait_placement.py [--root DIR] [--marks-only] > profiles/<tag>_probe_wait_placement.txt
tests/test_probe_wait_placement_cpu.py asserts on analyse_marks()."""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S"]
FUNC = re.compile(r"^(_ZN3mrp2ct13compactSearchILb([01])ELb([01])ELb([01])ENS0_7TierCfgILj(\d+)E\w*):")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
VMEM = ("global_", "buffer_", "flat_", "scratch_")


def compile_asm(root, out, marks):
    src = os.path.join(root, "libmultirobotplanning_amd", "csrc")
    cmd = [HIPCC] + FLAGS + ["-I", os.path.join(root, "include")] + (["-DMRP_CT_ASM_MARKS"] if marks else []) + ["ll_kernel.hip", "-o", out]
    return subprocess.Popen(cmd, cwd=src, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


def instances(lines):
    """[(name, (eps, plds, bg, wide), first line, end line)] of the compactSearch instances in the assembly."""
    found, cur = [], None
    for i, l in enumerate(lines):
        m = FUNC.match(l)
        if m:
            cur = (m.group(1), (m.group(2) == "1", m.group(3) == "1", m.group(4) == "1", int(m.group(5)) > 4), i)
        elif cur and l.startswith(".Lfunc_end"):
            found.append(cur + (i,))
            cur = None
    return found


def label_of(inst):
    eps, plds, bg, wide = inst
    return "compactSearch<%s, %s, %s, %s>" % ("true" if eps else "false", "true" if plds else "false", "true" if bg else "false",
                                                "Wide" if wide else "Narrow")


class Func:
    def __init__(self, lines, lo, hi):
        self.lines, self.lo, self.hi = lines, lo, hi
        self.labels = {}
        for i in range(lo, hi):
            m = LABEL.match(lines[i])
            if m:
                self.labels[m.group(1)] = i

    def insn(self, i):
        m = INSN.match(self.lines[i])
        return (m.group(1), m.group(2)) if m else None

    def mark(self, i):
        m = re.match(r"^\s*; PHASE (\d+)\s*$", self.lines[i])
        return int(m.group(1)) if m else None

    def walk(self, load, stop_at_mark):
        """Breadth first over the control flow from the instruction behind `load`.  Returns (any_wait, own_wait, reached):
        any_wait — some path meets an s_waitcnt vmcnt before it ends; own_wait — (instructions, LDS instructions) of the
        shortest path to a wait that waits for the load itself, or None; reached — a path gets to the stop mark.  A path
        ends at the stop mark (stop_at_mark), at a wait for the load, at a return or call, and at the function's end."""
        start = (load + 1, 0, 0, 0)  # line, vector-memory instructions behind the load (capped), instructions, LDS instructions
        seen, queue = {(load + 1, 0)}, collections.deque([start])
        any_wait, own_wait, reached = False, None, False

        def push(i, k, n, d):
            if (i, k) not in seen and self.lo <= i < self.hi:
                seen.add((i, k))
                queue.append((i, k, n, d))

        while queue:
            i, k, n, d = queue.popleft()
            if i >= self.hi:
                continue
            if stop_at_mark is not None and self.mark(i) == stop_at_mark:
                reached = True
                continue
            ins = self.insn(i)
            if ins is None:
                push(i + 1, k, n, d)
                continue
            op, rest = ins
            n += 1
            if op.startswith("ds_"):
                d += 1
            if op == "s_waitcnt":
                m = VMCNT.search(rest)
                if m:
                    any_wait = True
                    if k >= int(m.group(1)):  # fewer than N + 1 younger ones: the counter cannot reach N while this load is out
                        if own_wait is None:
                            own_wait = (n - 1, d)
                        continue
            if op.startswith(VMEM):
                k = min(k + 1, 64)
            if op in ("s_endpgm", "s_setpc_b64", "s_swappc_b64"):
                continue
            if op == "s_branch":
                push(self.labels.get(rest.strip(), self.hi), k, n, d)
                continue
            if op.startswith("s_cbranch"):
                push(self.labels.get(rest.strip().split()[-1], self.hi), k, n, d)
            push(i + 1, k, n, d)
        return any_wait, own_wait, reached


def analyse_marks(lines):
    """{instance tuple: dict(loads, followed, waited, in_flight)} for the EPS && !PLDS instances of a marks build."""
    res = {}
    for name, inst, lo, hi in instances(lines):
        if not inst[0] or inst[1]:
            continue
        f = Func(lines, lo, hi)
        r = dict(loads=0, followed=0, waited=0, in_flight=0, saveexec=0)
        p0 = None
        region = []
        for i in range(lo, hi):
            k = f.mark(i)
            if k == 0:
                p0, region = i, []
            elif k == 2 and p0 is not None:
                for j in region:
                    any_wait, own, reached = f.walk(j, 2)
                    assert reached or own is not None, (name, j)  # every path ends at the pop or at a wait for the load
                    r["loads"] += 1
                    r["followed"] += int(any_wait)
                    r["waited"] += int(own is not None)
                    r["in_flight"] += int(own is None)
                r["saveexec"] += sum(1 for j in range(p0, i) if (f.insn(j) or ("",))[0].startswith("s_and_saveexec"))
                p0 = None
            elif p0 is not None and (f.insn(i) or ("",))[0] == "global_load_ushort":
                region.append(i)
        res[inst] = r
    return res


def analyse_product(lines):
    """{instance tuple: [(instructions, LDS instructions) to the first wait for each global_load_ushort]}, product build."""
    res = {}
    for name, inst, lo, hi in instances(lines):
        if not inst[0] or inst[1]:
            continue
        f = Func(lines, lo, hi)
        res[inst] = [f.walk(i, None)[1] for i in range(lo, hi) if (f.insn(i) or ("",))[0] == "global_load_ushort"]
    return res


def build_and_read(root, marks_only=False):
    tmp = tempfile.mkdtemp(prefix="probe_wait_")
    try:
        jobs = [(os.path.join(tmp, "marks.s"), True)] + ([] if marks_only else [(os.path.join(tmp, "product.s"), False)])
        procs = [compile_asm(root, out, marks) for out, marks in jobs]
        errs = [p.communicate()[1].decode(errors="replace") for p in procs]
        for p, err in zip(procs, errs):
            if p.returncode != 0:
                raise RuntimeError("hipcc failed (exit %d):\n%s" % (p.returncode, err[-3000:]))
        return [open(out).read().split("\n") for out, _ in jobs]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def report(marks, product=None):
    out = []
    for inst in sorted(marks):
        r = marks[inst]
        out.append("%s  (marks build, PHASE 0 .. PHASE 2)" % label_of(inst))
        out.append("  row loads %d: %d waited before the pop, %d in flight at the pop; %d followed by some s_waitcnt vmcnt; %d s_and_saveexec"
                   % (r["loads"], r["waited"], r["in_flight"], r["followed"], r["saveexec"]))
        if product is not None:
            for n, w in enumerate(product.get(inst, [])):
                out.append("  product build, row load %d: %s" % (n, "never waited for inside the function" if w is None else
                                                                "%d instructions, %d of them LDS, to the first wait for it" % w))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--marks-only", action="store_true")
    a = ap.parse_args()
    asm = build_and_read(a.root, a.marks_only)
    print(report(analyse_marks(asm[0]), None if a.marks_only else analyse_product(asm[1])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
