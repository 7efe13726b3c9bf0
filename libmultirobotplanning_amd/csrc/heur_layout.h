// What the host (mrp_ll_compute_heuristics) and the BFS wave program (heur_bfs.h) agree on: the per-table descriptor and
// the LDS each form of the program needs.  Plain C++, no wave vocabulary.
#pragma once
#include <stdint.h>

namespace mrp {
namespace hb {

struct HeurJob {      // one table; what the host stages per goal
  uint32_t mapOff;    // word offset of the map's bitmap inside the maps buffer
  uint32_t tabOff;    // word offset of the table (a multiple of 32: its own 128-byte lines)
  uint32_t dims;      // dimx | dimy << 8
  uint32_t goal;      // x | y << 8
};

constexpr uint32_t kSmallLdsBytes = 2048;  // bfsSmall: the [32][32] halfword image of the table
constexpr bool isSmall(uint32_t dimx, uint32_t dimy) { return dimx <= 32u && dimy <= 32u; }
// bfsLarge: five bitmaps of the map's words rounded up to whole waves (available, column 0, last column, frontier, next
// frontier): 40 KB for 255 x 255
constexpr uint32_t largeLdsBytes(uint32_t dimx, uint32_t dimy) {
  return 5u * 4u * ((((dimx * dimy + 31u) >> 5) + 63u) & ~63u);
}
constexpr uint32_t ldsBytes(uint32_t dimx, uint32_t dimy) {
  return isSmall(dimx, dimy) ? kSmallLdsBytes : largeLdsBytes(dimx, dimy);
}

struct LookupJob {    // mrp_ll_heuristic_lookup: one entry of one table
  uint32_t tabOff;    // word offset of the table
  uint32_t half;      // halfword index inside it
};

}  // namespace hb
}  // namespace mrp
