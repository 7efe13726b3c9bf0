// TEST INFRASTRUCTURE — the one-search-per-call driver of emu_ll.cpp (the compact tier, libmultirobotplanning_amd/csrc/
// ll_compact.h, against wave_emu.h) with ll_compact.h's counting hook defined: what the expansions of a search did, beside
// what they gave.  Built by tests/test_expansion_emu_cpu.py twice — as the tier is and with -DMRP_CT_PLAIN_EXPANSION (no erase
// at the root, no grid of focal counts) — into tests/_build/libemu_expansion*.so; never part of the product.
#include <stdint.h>

// 0 erases at the root, 1 group reads of the erase scan, 2 / 3 expansions whose focal counts took the grid / the loop,
// 4 erases at a position from 256 on, 5 erases of the open array's last element, 6 erases at the root of an open list of more
// than 512 entries
static int64_t g_expansion_counts[8];
#define MRP_CT_COUNT(k, v) (g_expansion_counts[k] += (int64_t)(v))

#include "emu_ll.cpp"  // emu_compact_search, as tests/test_compact_emu.py's emu_search calls it

extern "C" {

// out[0..7] = the counters since the last reset; reset != 0: back to zero afterwards
void emu_expansion_counts(int64_t* out, int reset) {
  for (int k = 0; k < 8; ++k) {
    out[k] = g_expansion_counts[k];
    if (reset) g_expansion_counts[k] = 0;
  }
}

}  // extern "C"
