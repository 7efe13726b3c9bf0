// One workgroup's slot of the device arena: its layout, once, for the host that sizes it (mrp_ll_create) and for every
// device search that runs in it.  Compiles alone under g++ (tests/support/slot_layout_check.cpp).  Byte map, n = arena_nodes:
//   0            node records, 16 bytes each                                                              nodeBytes(n)
//   nodeBytes    open, focal, walk queue: 8-byte bias slot, n 64-bit entries, 8 bytes of slack each     3 * heapBytes(n)
//   areaBytes    (time, cell) bitmap: max_horizon rows of row_words words                                bitsBytes
//   scratchOff   path out: max_horizon halfwords (SIPP: a word per state, as far as they fit)           outBytes       (256 | scratchOff)
//   consCopy     constraint copy: kConsLocalWords words (stageConstraints / stageConstraintSet)          consBytes
//   pathsCopy    path-table copy: a job's focal table, a root chain's table (runChain; read again by scanNode), runSipp's
//                safe-interval table (16-byte copies: aligned for max_horizon % 8 == 0)                   arena_paths_bytes
//   stride                                                                                                              (256 | stride)
// What overlays [0, areaBytes), each while no other search of the slot is live:
//   cutArena (runJob's arena tier, runSipp)  the map as it stands; runSipp's status words take the bitmap
//   runTaArena                                nodes and open list as above, its status table in the focal + walk areas
//   runJobTaEps                               its own cut: status table, node records A and B, three heaps (ll_ta.h)
//   compact tiers                             cameFrom table at 0, behind it the BG bitmap (ll_jobs.h compactFits / baseCJob)
#ifndef MRP_LL_SLOT_H
#define MRP_LL_SLOT_H
#include <stdint.h>

#include "ll_device.h"
#ifdef __HIP__  // (the language mode of hipcc: a .hip source, device and host pass)
#define MRP_SLOT_FN __host__ __device__ inline
#else
#define MRP_SLOT_FN inline
#endif

namespace mrp {
namespace slot {
MRP_SLOT_FN uint64_t align256(uint64_t v) { return (v + 255) & ~255ull; }
MRP_SLOT_FN uint64_t nodeBytes(uint32_t arenaNodes) { return (uint64_t)arenaNodes * 16; }
MRP_SLOT_FN uint64_t heapBytes(uint32_t arenaNodes) { return (uint64_t)arenaNodes * 8 + 16; }
MRP_SLOT_FN uint64_t areaBytes(uint32_t arenaNodes) { return nodeBytes(arenaNodes) + 3 * heapBytes(arenaNodes); }
MRP_SLOT_FN uint64_t bitsBytes(uint32_t maxHorizon, uint32_t rowWords) { return (uint64_t)maxHorizon * rowWords * 4; }
MRP_SLOT_FN uint64_t outBytes(uint32_t outStride) { return (uint64_t)outStride * 2; }
MRP_SLOT_FN uint64_t consBytes() { return (uint64_t)kConsLocalWords * 4; }
MRP_SLOT_FN uint64_t scratchOff(uint32_t arenaNodes, uint32_t maxHorizon, uint32_t rowWords) {
  return align256(areaBytes(arenaNodes) + bitsBytes(maxHorizon, rowWords));
}
MRP_SLOT_FN uint64_t stride(uint32_t arenaNodes, uint32_t maxHorizon, uint32_t rowWords, uint32_t arenaPathsBytes) {
  return align256(scratchOff(arenaNodes, maxHorizon, rowWords) + outBytes(maxHorizon) + consBytes() + arenaPathsBytes);
}
// The three scratch areas of the slot at `s` (LaunchParams::arena_scratch_off, ::out_stride)
MRP_SLOT_FN uint16_t* outPath(uint8_t* s, uint32_t scratchOff, uint32_t /*outStride*/) { return (uint16_t*)(s + scratchOff); }
MRP_SLOT_FN uint32_t* consCopy(uint8_t* s, uint32_t scratchOff, uint32_t outStride) { return (uint32_t*)(s + scratchOff + outBytes(outStride)); }
MRP_SLOT_FN uint8_t* pathsCopy(uint8_t* s, uint32_t scratchOff, uint32_t outStride) { return s + scratchOff + outBytes(outStride) + consBytes(); }
}  // namespace slot
}  // namespace mrp
#endif  // MRP_LL_SLOT_H
