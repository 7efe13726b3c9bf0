// TEST INFRASTRUCTURE — a stand-alone check of the arena slot's layout (libmultirobotplanning_amd/csrc/ll_slot.h), built by
// tests/test_slot_layout_cpu.py with the host sanitizers and run as a program of its own.  For every option set the slot is a
// heap block of exactly slot::stride bytes and each scratch area is filled through its accessor, so AddressSanitizer sees an
// area that reaches past the slot and the read-back sees two that overlap.  Expected numbers are the formula mrp_ll_create
// used before the header existed, restated here, and three results worked by hand.  Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../libmultirobotplanning_amd/csrc/ll_slot.h"

namespace slot = mrp::slot;

#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::fprintf(stderr, "slot_layout_check: line %d: %s  (arena_nodes %u, max_horizon %u, max_cells %u)\n", __LINE__, \
                   #cond, gNodes, gHorizon, gCells);                                                                   \
      std::exit(1);                                                                                                    \
    }                                                                                                                  \
  } while (0)

namespace {

uint32_t gNodes, gHorizon, gCells;
constexpr uint32_t kPathsBytes = 128 * 1024;  // mrp_ll_create's path-table copy

void checkOne(uint32_t nodes, uint32_t horizon, uint32_t cells) {
  gNodes = nodes; gHorizon = horizon; gCells = cells;
  const uint32_t rowWords = (cells + 31u) / 32u;
  // the formula as mrp_ll_create wrote it out
  uint64_t want = static_cast<uint64_t>(nodes) * 16 + 3ull * (static_cast<uint64_t>(nodes) * 8 + 16) +
                  static_cast<uint64_t>(horizon) * rowWords * 4;
  want = (want + 255) & ~255ull;
  const uint64_t wantOff = want;
  want += static_cast<uint64_t>(horizon) * 2 + 2048 * 4 + kPathsBytes;
  want = (want + 255) & ~255ull;
  const uint64_t off = slot::scratchOff(nodes, horizon, rowWords), stride = slot::stride(nodes, horizon, rowWords, kPathsBytes);
  CHECK(off == wantOff && stride == want);
  CHECK(off <= 0xFFFFFFFFull);  // LaunchParams::arena_scratch_off has 32 bits

  // the areas in front of the scratch tail: in order, back to back
  CHECK(slot::nodeBytes(nodes) == 16ull * nodes && slot::heapBytes(nodes) == 8ull * nodes + 16);
  CHECK(slot::areaBytes(nodes) == slot::nodeBytes(nodes) + 3 * slot::heapBytes(nodes));
  CHECK(slot::bitsBytes(horizon, rowWords) == 4ull * horizon * rowWords);
  CHECK(slot::areaBytes(nodes) + slot::bitsBytes(horizon, rowWords) <= off && off % 256 == 0 && stride % 256 == 0);

  // the scratch tail, through the accessors the device code uses (out_stride == max_horizon)
  std::unique_ptr<uint8_t[]> block(new uint8_t[stride]);
  uint8_t* base = block.get();
  uint8_t* out = reinterpret_cast<uint8_t*>(slot::outPath(base, static_cast<uint32_t>(off), horizon));
  uint8_t* cons = reinterpret_cast<uint8_t*>(slot::consCopy(base, static_cast<uint32_t>(off), horizon));
  uint8_t* paths = slot::pathsCopy(base, static_cast<uint32_t>(off), horizon);
  CHECK(out == base + off);
  CHECK(cons == out + slot::outBytes(horizon) && slot::outBytes(horizon) == 2ull * horizon);
  CHECK(paths == cons + slot::consBytes() && slot::consBytes() == 4ull * mrp::kConsLocalWords);
  CHECK(paths + kPathsBytes <= base + stride);
  std::memset(out, 1, slot::outBytes(horizon));
  std::memset(cons, 2, slot::consBytes());
  std::memset(paths, 3, kPathsBytes);
  CHECK(out[0] == 1 && out[slot::outBytes(horizon) - 1] == 1 && cons[0] == 2 && cons[slot::consBytes() - 1] == 2 && paths[0] == 3 &&
        paths[kPathsBytes - 1] == 3);

  // alignment, relative to the slot (slots start at multiples of 256 of a hipMalloc block).  The constraint copy holds words
  // and runSipp copies its table in 16-byte units; both follow max_horizon halfwords, so at HEAD the first holds for an even
  // max_horizon and the second for a multiple of 8 — not for max_horizon = 1, where both areas start 2 bytes past a multiple
  // of 256.  Recorded, not changed: the layout is the parent's.
  CHECK((cons - base) % 4 == (horizon % 2 ? 2 : 0));
  CHECK((paths - base) % 16 == (horizon * 2) % 16);
  if (horizon % 8 == 0) CHECK((cons - base) % 4 == 0 && (paths - base) % 16 == 0);
}

}  // namespace

int main() {
  const uint32_t nodes[] = {131072, 4096, 2}, horizons[] = {512, 1, 1024}, cells[] = {4096, 1, 65025};
  for (uint32_t n : nodes)
    for (uint32_t h : horizons)
      for (uint32_t c : cells) checkOne(n, h, c);
  // by hand.  The defaults: 131072 * 16 + 3 * (131072 * 8 + 16) = 5 242 928, + 512 * 128 * 4 = 5 505 072 -> 5 505 280;
  // + 1024 + 8192 + 131072 = 5 645 568, a multiple of 256 as it stands
  gNodes = 131072; gHorizon = 512; gCells = 4096;
  CHECK(slot::scratchOff(131072, 512, 128) == 5505280ull && slot::stride(131072, 512, 128, kPathsBytes) == 5645568ull);
  // the smallest: 2 * 16 + 3 * 32 = 128, + 4 = 132 -> 256; + 2 + 8192 + 131072 = 139 522 -> 139 776
  gNodes = 2; gHorizon = 1; gCells = 1;
  CHECK(slot::scratchOff(2, 1, 1) == 256ull && slot::stride(2, 1, 1, kPathsBytes) == 139776ull);
  // 4096 nodes, 1024 rows of 2033 words: 65 536 + 3 * 32 784 = 163 888, + 8 327 168 = 8 491 056 -> 8 491 264;
  // + 2048 + 8192 + 131072 = 8 632 576 -> 8 632 576 (33 721 * 256)
  gNodes = 4096; gHorizon = 1024; gCells = 65025;
  CHECK(slot::scratchOff(4096, 1024, 2033) == 8491264ull && slot::stride(4096, 1024, 2033, kPathsBytes) == 8632576ull);
  std::printf("slot_layout_check: ok\n");
  return 0;
}
