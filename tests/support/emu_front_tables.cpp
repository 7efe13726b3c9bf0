// TEST INFRASTRUCTURE — sequences of compact-tier searches (libmultirobotplanning_amd/csrc/ll_compact.h, the code the gfx950
// kernels run, against the host interpretation of its wave vocabulary, wave_emu.h) in the two places the A*-epsilon-only
// kernels keep a search's focal path table: behind the LDS window (PLDS = true) and in "device memory" (PLDS = false,
// CJob::pathsG), which is where the front workgroups of mrp_ll_session_front_tables keep it.
// Built by tests/test_front_tables_emu_cpu.py into tests/_build/libemu_front_tables.so; never part of the product.
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "wave_emu.h"
#include "../../libmultirobotplanning_amd/csrc/ll_compact.h"

extern "C" {

// Agents 0 .. n_agents - 1 of one instance, one search each, every search against the paths found before it — what a root
// chain does (ll_jobs.h runChain).  rows = 64: the chain's own table [64][npad], which gains one column per path and is never
// rebuilt; rows = 0: the table of a conflict-tree child (runJob), put together for every search with as many rows as the
// longest earlier path has cells (row tPad - 1 repeats for ever: the search clamps to it).  in_memory = 0: the table is
// copied behind the window before each search; 1: the window holds no table and the search reads `table` itself.
// budget < 0: unlimited, else the expansions all searches share (each gets what is left; the sequence ends with the first
// search that has no path).  The sequence also ends in front of a search that outgrows the tier (nothing recorded for it).
// Per search k: out[8 k ..] = status, cost, fmin, n_states, expanded, nodes, out-of-window LDS reads, out-of-window LDS
// writes; cells[64 k ..] = the path (x | y << 8), 0xFFFF beyond its end; heaps[heap_words k ..] = the open and the focal
// area of the window as the search left them.  Returns the number of searches recorded, or -2 for an input out of range.
int emu_front_chain(int in_memory, int rows, int dimx, int dimy, int n_obst, const int32_t* obst_xy, int n_agents,
                    const int32_t* starts_goals_xy, float w, int64_t budget, int64_t* out, int32_t* cells, uint32_t* heaps,
                    int heap_words) {
  using namespace mrp::ct;
  if (dimx < 1 || dimy < 1 || dimx > 32 || dimy > 32 || n_agents < 1 || n_agents > 128 || (rows != 0 && rows != 64)) return -2;
  if (heap_words != (int)(2u * kHeapBytes / 4u)) return -2;
  const uint32_t cellsN = (uint32_t)dimx * dimy;
  std::vector<uint32_t> obst((cellsN + 31) / 32, 0u);
  for (int i = 0; i < n_obst; ++i) {
    const int x = obst_xy[2 * i], y = obst_xy[2 * i + 1];
    if (x < 0 || x >= dimx || y < 0 || y >= dimy) continue;
    const uint32_t c = (uint32_t)(y * dimx + x);
    obst[c >> 5] |= 1u << (c & 31);
  }
  const uint32_t npad = ((uint32_t)n_agents + 15u) & ~15u;
  std::vector<std::vector<uint16_t>> paths((size_t)n_agents);
  std::vector<uint16_t> table;
  const uint32_t none = 0;
  int done = 0;
  for (int a = 0; a < n_agents; ++a) {
    // the table of this search: [tpad][npad], 0xFFFF = nobody, every path extended by its last cell
    uint32_t tpad = (uint32_t)rows;
    if (rows == 0)
      for (int b = 0; b < a; ++b) tpad = std::max<uint32_t>(tpad, (uint32_t)paths[b].size());
    const uint32_t np = tpad ? npad : 0u;
    table.assign((size_t)tpad * np + 256, 0xFFFFu);  // (lanes beyond a row's end are masked, but keep reads in bounds)
    for (int b = 0; b < a; ++b)
      for (uint32_t t = 0; t < tpad && !paths[b].empty(); ++t)
        table[(size_t)t * np + b] = paths[b][std::min<size_t>(t, paths[b].size() - 1)];
    const uint32_t tableBytes = tpad * np * 2u;
    const bool plds = !in_memory || tableBytes == 0u;  // (no table at all: runJob runs the instance that reads none)
    std::vector<uint8_t> ldsMem(windowBytes(true) + (in_memory ? 0u : tableBytes), 0xA5);  // garbage from "the previous job"
    wv::LdsWindow win{ldsMem.data(), (uint32_t)ldsMem.size(), 0, 0};
    if (!in_memory && tableBytes) std::memcpy(ldsMem.data() + pathsOff(true), table.data(), tableBytes);
    std::vector<uint8_t> parentTab(kParentBytes, 0xEE);
    std::vector<uint32_t> bitsG(kBitsBytes / 4u, 0xA5A5A5A5u);
    std::vector<uint16_t> outPath(1024, 0);
    const int32_t* q = starts_goals_xy + 4 * a;
    CJob J;
    std::memset(&J, 0, sizeof(J));
    J.dimx = dimx; J.dimy = dimy; J.sx = q[0]; J.sy = q[1]; J.gx = q[2]; J.gy = q[3];
    J.lastGoal = -1;
    J.w = w;
    J.vc = (uint64_t)(uintptr_t)&none; J.ec = (uint64_t)(uintptr_t)&none;
    J.obst = (uint64_t)(uintptr_t)obst.data(); J.obstWords = (uint32_t)obst.size();
    J.nAgentsPad = np; J.tPad = tpad;
    J.pathsG = in_memory ? (uint64_t)(uintptr_t)table.data() : 0ull;
    J.maxExp = budget < 0 ? 0xFFFFFFFFu : (uint32_t)std::min<int64_t>(budget, 0xFFFFFFFEll);
    J.openCap = kCap; J.maxT = kMaxT;
    J.parentTab = (uint64_t)(uintptr_t)parentTab.data();
    J.outPath = (uint64_t)(uintptr_t)outPath.data();
    J.bitsG = (uint64_t)(uintptr_t)bitsG.data();
    std::memcpy(ldsMem.data() + oJob, &J, sizeof(J));
    const int32_t rc = plds ? compactSearch<true, true, true>(&win) : compactSearch<true, false, true>(&win);
    CRes R;
    std::memcpy(&R, ldsMem.data() + oRes, sizeof(R));
    if (rc != R.status) return -3;
    if (rc == C_OVERFLOW) break;
    int64_t* o = out + 8 * done;
    o[0] = rc; o[1] = R.cost; o[2] = R.fmin; o[3] = R.nStates; o[4] = R.expanded; o[5] = R.nodes;
    o[6] = (int64_t)win.oobReads; o[7] = (int64_t)win.oobWrites;
    for (int k = 0; k < 64; ++k) cells[64 * done + k] = (rc == C_OK && k < R.nStates) ? outPath[k] : 0xFFFF;
    std::memcpy(heaps + (size_t)heap_words * done, ldsMem.data() + oOpen, (size_t)heap_words * 4u);
    done += 1;
    if (rc != C_OK) break;
    if (R.nStates < 1 || R.nStates > 64) return -3;
    paths[a].assign(outPath.begin(), outPath.begin() + R.nStates);
    if (budget >= 0) budget = budget > (int64_t)R.expanded ? budget - (int64_t)R.expanded : 0;
  }
  return done;
}

}  // extern "C"
