"""The lane mask of the focal-table row loads, on the CPU emulator (tests/support/emu_ll.cpp through tests/test_compact_emu.py's
loader: ll_compact.h, the kernels' own source, against tests/support/wave_emu.h).

compactSearch with the table in memory (PLDS = false) loads the rows t and t + 1 unmasked — a lane beyond the row's end reads
the row's last column — and leaves those lanes out where the loaded cells are counted.  The emulator has no unmasked loads:
ll_compact.h falls back to the masked ones with every lane on, so the emulator reads every lane as the device does.
tests/row_wait_cases.py has the searches; each runs in the three instances that read the table from memory — the narrow geometry
with the bitmap in memory (what the front workgroups run), the wide one (the heavy workgroups) and the narrow one with the bitmap
in LDS (the mixed kernels) — and must equal the oracle in every result field and in the path, without an access outside the window.

A build of ll_compact.h with `valid0` / `valid1` replaced by all ones (the ballot mask left out) fails n16, n32, n80, clamp
and constraints in all three instances — n16, n32, n80: 38 expansions instead of 36, another path; clamp: 39 instead of 37;
constraints: cost 11 after 57 expansions instead of cost 10 after 52 — and passes n2, n10, n64, n66 and n128: the engine pads a
table to a multiple of 16 columns, so at 2, 10 and 66 agents the last column is empty, and at 64 and 128 no lane is clamped.
test_the_cases_cover_the_clamped_lanes pins that the set holds sensitive cases for either row load."""
import pytest

import row_wait_cases as rw
import test_compact_emu as ce

C_OK = 0


@pytest.fixture(scope="module")
def lib(oracle_mod):
    return ce._emu_lib()


FORMS = {"narrow": (True, False), "wide": (True, True), "narrow_lds_bitmap": (False, False)}  # (bitmap in memory, wide)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", rw.NAMES)
def test_search_equals_the_oracle(lib, name, form):
    c = rw.case(name)
    lib._bg, lib._wide = FORMS[form]
    inst = c["inst"]
    r = ce.emu_search(lib, True, inst, c["agent"], inst["starts"][0], inst["goals"][0], c["vc"], c["ec"], c["ctx_paths"], rw.W,
                      lds_path_bytes=0)  # no room in the window: the table is read from memory
    want = rw.expected(c)
    print(name, form, {k: r[k] for k in ("status", "cost", "fmin", "n_states", "expanded")},
          {k: want[k] for k in ("cost", "fmin", "n_states", "expanded")})
    assert (r["oob_reads"], r["oob_writes"]) == (0, 0)
    assert r["status"] == C_OK  # (a search of the tier: not handed over)
    assert {k: r[k] for k in ("status", "cost", "fmin", "n_states", "expanded")} == {k: want[k] for k in ("status", "cost", "fmin", "n_states", "expanded")}
    assert r["states"] == [s[1:] for s in want["states"]]


def test_the_cases_cover_the_clamped_lanes():
    """What makes a case sensitive (row_wait_cases.py): clamped lanes and a real agent in the last column, whose path lies
    on agent 0's upper way — in the first row load (16, 32 columns) and in the second (80)."""
    sens = [c for c in rw.cases() if c["sensitive"]]
    assert {c["n"] for c in sens} == {16, 32, 80}
    for c in sens:
        last = c["ctx_paths"][c["n"] - 1]
        assert len(last) >= 2 and c["agent"] != c["n"] - 1
        assert any(y == 1 and 2 <= x <= 9 for x, y in last[1:]), c["name"]  # on agent 0's upper way, at some t + 1
    clamp = rw.case("clamp")
    assert max(len(p) for p in clamp["ctx_paths"]) == 2 < len(clamp["want"]["states"])  # t >= tPad - 1 from the first step on
    cons = rw.case("constraints")
    assert cons["vc"] and cons["ec"] and cons["want"]["expanded"] != rw.case("n16")["want"]["expanded"]
