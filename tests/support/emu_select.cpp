// TEST INFRASTRUCTURE — the one-search-per-call driver of emu_ll.cpp (the compact tier, libmultirobotplanning_amd/csrc/
// ll_compact.h, against wave_emu.h) with ll_compact.h's counting hook defined, room for the counters of the search loop's
// exits, and the hook at the end of a search, which keeps a copy of the LDS window as the search left it.  Built by
// tests/test_select_stores_emu_cpu.py — as the tier is, with -DMRP_CT_EXEC_STORES, with -DMRP_CT_PLAIN_LOOP, with both and
// with -DMRP_CT_PLAIN_EXPANSION — into tests/_build/libemu_select*.so, and by tests/support/select_sanitize_main.cpp into a
// stand-alone program; never part of the product.
#include <stdint.h>

#include <vector>

//  0 .. 30 as in emu_push.cpp
// 31 goal pops                                  32 ... of the start node (start equals goal)
// 33 searches whose open list ran empty         34 pops of the goal cell at t <= lastGoal (no goal: the node expands)
// 35 exits at the expansion cap                 36 / 37 / 38 overflows: open entries, t > maxT, the focalH field
// 39 walks that outgrew their queue             40 pops that empty a list
// 41 / 42 pops that leave more than 31 / 63 entries in exactly one of the two lists (the other side of the second / third
//         descend block idles)                  43 pops of a list of 32, 33, 64 or 65 entries
// 44 turns with one push into the open list and none into the focal list
#define MRP_CT_COUNT_SLOTS 48
static int64_t g_select_counts[MRP_CT_COUNT_SLOTS];
#define MRP_CT_COUNT(k, v) (g_select_counts[k] += (int64_t)(v))
static std::vector<uint8_t> g_select_window;
#define MRP_CT_DONE(lds) g_select_window.assign((lds)->mem, (lds)->mem + (lds)->size)

#include "emu_ll.cpp"  // emu_compact_search, emu_compact_search_ta

extern "C" {

// out[0..47] = the counters since the last reset; reset != 0: back to zero afterwards
void emu_select_counts(int64_t* out, int reset) {
  for (int k = 0; k < MRP_CT_COUNT_SLOTS; ++k) {
    out[k] = g_select_counts[k];
    if (reset) g_select_counts[k] = 0;
  }
}

// the window of the last search, as it was when the search returned: its size; the first min(size, cap) bytes go to out
int emu_select_window(uint8_t* out, int cap) {
  const int n = (int)g_select_window.size();
  for (int i = 0; i < n && i < cap; ++i) out[i] = g_select_window[(size_t)i];
  return n;
}

// where the scratch word of the select-address stores lies (the one word that may differ between builds)
int emu_select_scratch_offset() { return (int)mrp::ct::oScratch; }

}  // extern "C"
