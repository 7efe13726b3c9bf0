"""Cases of the expansion's push step and of the heap roots kept in a register (ll_compact.h pushTurn, compactSearch's `tops`;
tests/test_push_emu_cpu.py on the CPU emulator, tests/test_push_gpu.py on the device).  HIP-free: the oracle alone.  A case is
one A*-epsilon search (w = 1.3) on a map of at most 32 x 32 cells with the oracle's answer, in the form of
tests/expansion_cases.py, whose cases (tests/row_wait_cases.py's among them) are the set:

  * corridor: one successor per turn, every push into an empty list (position 0);
  * five_a0, five_a8: five successors, all within the focal bound — turns of 2 + 2 + 1 with rows 2 and 3 both — and two
    successors with equal open keys;
  * open512: chains of nine and ten ancestors;  erase_last: the erase of the open array's last element;
  * n32 .. n128: the loop of focal counts;
  * two_open (this file's own): a corridor of three cells, (0, 0) to (2, 0).  The first expansion pushes Wait and Right as a
    pair; the second pops Right, the open list's root, with Wait the only other entry — the pop whose new OPEN root is the
    re-inserted last element, which no search of the golden trees has (there the root's children are always better).

What the golden conflict trees add (every class of tests/test_push_emu_cpu.py's counters is met by these and the trees
together; the test says so, class by class) is listed there."""
import expansion_cases as ex

W = ex.W
OWN = ("two_open",)
NAMES = ex.NAMES + OWN
_CASES = None


def _two_open():
    inst = dict(dimx=3, dimy=1, obstacles=[], starts=[[0, 0]], goals=[[2, 0]])
    return ex._case("two_open", inst, 0, [[]])


def cases():
    global _CASES
    if _CASES is None:
        _CASES = list(ex.cases()) + [_two_open()]
        assert tuple(c["name"] for c in _CASES) == NAMES
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


def expected(c):
    return ex.expected(c)


def dump(path):
    """The cases as numbers, for tests/support/push_sanitize_main.cpp (the format is described there)."""
    with open(path, "w") as f:
        for c in cases():
            inst, a, want = c["inst"], c["agent"], expected(c)
            flat = lambda rows: [v for r in rows for v in r]  # noqa: E731
            n = [inst["dimx"], inst["dimy"], len(inst["obstacles"])] + flat(inst["obstacles"]) + inst["starts"][a] + inst["goals"][a]
            n += [len(c["vc"])] + flat(c["vc"]) + [len(c["ec"])] + flat(c["ec"]) + [len(c["ctx_paths"]), a]
            n += [len(p) for p in c["ctx_paths"]] + flat(flat(c["ctx_paths"]))
            n += [want[k] for k in ("status", "cost", "fmin", "n_states", "expanded")]
            f.write(c["name"] + " " + " ".join(str(int(v)) for v in n) + "\n")


if __name__ == "__main__":
    import sys
    dump(sys.argv[1])
