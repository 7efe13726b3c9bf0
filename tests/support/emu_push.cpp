// TEST INFRASTRUCTURE — the one-search-per-call driver of emu_ll.cpp (the compact tier, libmultirobotplanning_amd/csrc/
// ll_compact.h, against wave_emu.h) with ll_compact.h's counting hook defined and room for the counters of the push step and
// of the kept heap roots.  Built by tests/test_push_emu_cpu.py — as the tier is, with -DMRP_CT_PLAIN_EXPANSION, with
// -DMRP_CT_KEEP_TOPS, with each part off alone, and with -DMRP_CT_CHECK_TOPS — into tests/_build/libemu_push*.so, and by
// tests/support/push_sanitize_main.cpp into a stand-alone program; never part of the product.
#include <stdint.h>

//  0 erases at the root                         7 bubbled erases
//  8 loop tops that compared the kept roots with the loaded ones (MRP_CT_CHECK_TOPS)      9 ... that found them different
// 10 / 11 pops whose new open root is the re-inserted last element / a pulled-up child    12 / 13 the same for the focal list
// 14 / 15 turns with one / two successors       16 / 17 / 18 expansions with three / four / five successors
// 19 turns with focal row 2 alone   20 with rows 2 and 3   21 pairs whose first successor is outside the bound, the second inside
// 22 / 23 pairs whose second chain is one level deeper, open / focal                      24 pushes into position 0
// 25 / 26 first pushes that become the root, open / focal      27 / 28 second pushes that displace such a first one
// 29 / 30 pushes whose key equals the root's, open / focal     (1 .. 6: as in emu_expansion.cpp)
#define MRP_CT_COUNT_SLOTS 32
static int64_t g_push_counts[MRP_CT_COUNT_SLOTS];
#define MRP_CT_COUNT(k, v) (g_push_counts[k] += (int64_t)(v))

#include "emu_ll.cpp"  // emu_compact_search, as tests/test_compact_emu.py's emu_search calls it

extern "C" {

// out[0..31] = the counters since the last reset; reset != 0: back to zero afterwards
void emu_push_counts(int64_t* out, int reset) {
  for (int k = 0; k < MRP_CT_COUNT_SLOTS; ++k) {
    out[k] = g_push_counts[k];
    if (reset) g_push_counts[k] = 0;
  }
}

}  // extern "C"
