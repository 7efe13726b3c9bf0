// TEST INFRASTRUCTURE — the table form of the compact search tier (libmultirobotplanning_amd/csrc/ll_compact.h
// compactSearch<EPS, PLDS, false, Narrow, true>: MRP_LL_JOB_TABLE_H, the code the gfx950 mixed kernels run) compiled against the
// host interpretation of its wave vocabulary (wave_emu.h), one search per call.  Built by tests/test_table_h_emu_cpu.py into
// tests/_build/libemu_table_h.so; never part of the product.
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "wave_emu.h"
#include "../../libmultirobotplanning_amd/csrc/ll_compact.h"
#include "../../libmultirobotplanning_amd/csrc/host/ll_pack.h"

namespace {
using mrp::host::fillFocalTable;
using mrp::host::focalTableRows;
using mrp::host::packEdgeWords;
using mrp::host::packVertexWords;
constexpr int kHorizon = 1024;
struct VecSink {
  std::vector<uint32_t>& v;
  void push(uint32_t w) { v.push_back(w); }
};
}  // namespace

extern "C" {

// One MRP_LL_JOB_TABLE_H search through the narrow tier (eps: 0 = A*, 1 = A*-epsilon).  Inputs as emu_compact_search's
// (tests/support/emu_ll.cpp), plus heur: the goal's shortest-path table, [dimy][dimx] int32 (INT32_MAX: unreachable), as the
// caller of mrp_ll_upload_heuristic passes it.  lds_path_bytes (>= 2048) = the window's path area: the focal table stands in
// it when it fits together with the 2048 bytes of the heuristic table, and is read from "device memory" otherwise — the
// launcher's rule (ll_jobs.h runJobTableH).
// out[0..5] = status (ct::C_*; -1: not a search of this tier), cost, fmin, n_states, expanded, nodes created; out[6] / out[7] =
// out-of-window LDS reads / writes; out[8] = 1 when the focal table stood in the window; out[9] = halfwords of the path
// buffer the search wrote.
int emu_table_h_search(int eps, int dimx, int dimy, int n_obst, const int32_t* obst_xy, int sx, int sy, int gx, int gy,
                       const int32_t* heur, float w, int n_vc, const int32_t* vc, int n_ec, const int32_t* ec, int n_agents,
                       int agent_idx, const int32_t* path_len, const int32_t* path_xy, int64_t max_exp, int lds_path_bytes,
                       int64_t* out, int32_t* states_xy, int states_cap) {
  using namespace mrp::ct;
  if (dimx < 1 || dimy < 1 || dimx > 32 || dimy > 32 || lds_path_bytes < 2048 || eps < 0 || eps > 1) return -2;
  const uint32_t cells = (uint32_t)dimx * dimy;
  std::vector<uint32_t> obst((cells + 31) / 32, 0u);
  for (int i = 0; i < n_obst; ++i) {
    const int x = obst_xy[2 * i], y = obst_xy[2 * i + 1];
    if (x < 0 || x >= dimx || y < 0 || y >= dimy) continue;
    const uint32_t c = (uint32_t)(y * dimx + x);
    obst[c >> 5] |= 1u << (c & 31);
  }
  std::vector<uint32_t> vcw, ecw;
  VecSink vcs{vcw}, ecs{ecw};
  const int lastGoal = packVertexWords(vc, n_vc, dimx, dimy, kHorizon, gx, gy, false, vcs);
  packEdgeWords(ec, n_ec, dimx, dimy, kHorizon, ecs);
  vcw.push_back(0);
  ecw.push_back(0);
  std::vector<uint16_t> table;
  uint32_t npad = 0, tpad = 0;
  if (eps && n_agents > 0) {
    std::vector<const int32_t*> pathOf((size_t)n_agents);
    size_t off = 0;
    for (int a = 0; a < n_agents; ++a) {
      pathOf[a] = path_xy + 2 * off;
      off += (size_t)std::max(path_len[a], 0);
    }
    const int tp = focalTableRows(n_agents, agent_idx, path_len);
    if (tp > 0) {
      npad = ((uint32_t)n_agents + 15u) & ~15u;
      tpad = (uint32_t)tp;
      table.resize((size_t)tpad * npad);
      fillFocalTable(table.data(), tp, npad, n_agents, agent_idx, path_len, pathOf.data(), dimx, dimy);
    }
  }
  if (npad > 128) return -2;
  const uint32_t tableBytes = tpad * npad * 2u;
  const bool tableInLds = tableBytes != 0 && tableBytes + 2048u <= (uint32_t)lds_path_bytes;
  std::vector<uint16_t> heurTab(1024, 0xFFFFu);  // [y * 32 + x], 0xFFFF = unreachable (what mrp_ll_upload_heuristic stores)
  for (int y = 0; y < dimy; ++y)
    for (int x = 0; x < dimx; ++x) {
      const int32_t d = heur[y * dimx + x];
      heurTab[y * 32 + x] = (d < 0 || d > 0xFFFE) ? 0xFFFFu : (uint16_t)d;
    }
  std::vector<uint8_t> ldsMem(windowBytes(false) + (uint32_t)lds_path_bytes, 0xA5);  // garbage from "the previous job"
  wv::LdsWindow win{ldsMem.data(), (uint32_t)ldsMem.size(), 0, 0};
  if (tableInLds) std::memcpy(ldsMem.data() + pathsOff(false), table.data(), tableBytes);
  std::vector<uint8_t> parentTab(kParentBytes, 0xEE);
  std::vector<uint16_t> outPath(1024, 0xBEEF);
  table.resize(table.size() + 256, 0xFFFFu);  // (lanes beyond a row's end are masked, but keep reads in bounds)
  CJob J;
  std::memset(&J, 0, sizeof(J));
  J.dimx = dimx; J.dimy = dimy; J.sx = sx; J.sy = sy; J.gx = gx; J.gy = gy;
  J.lastGoal = lastGoal;
  J.w = w;
  J.nVc = (uint32_t)vcw.size() - 1; J.nEc = (uint32_t)ecw.size() - 1;
  J.vc = (uint64_t)(uintptr_t)vcw.data(); J.ec = (uint64_t)(uintptr_t)ecw.data();
  J.obst = (uint64_t)(uintptr_t)obst.data(); J.obstWords = (uint32_t)obst.size();
  J.nAgentsPad = npad; J.tPad = tpad;
  J.pathsG = (uint64_t)(uintptr_t)table.data();
  J.maxExp = max_exp < 0 ? 0xFFFFFFFFu : (uint32_t)std::min<int64_t>(max_exp, 0xFFFFFFFEll);
  J.openCap = kCap;
  J.maxT = kMaxT;
  J.parentTab = (uint64_t)(uintptr_t)parentTab.data();
  J.outPath = (uint64_t)(uintptr_t)outPath.data();
  J.bitsG = (uint64_t)(uintptr_t)heurTab.data();  // the table form's use of the field
  if (J.nEc > 64) return -2;
  std::memcpy(ldsMem.data() + oJob, &J, sizeof(J));
  const int32_t rc = !eps         ? compactSearch<false, true, false, Narrow, true>(&win)
                     : tableInLds ? compactSearch<true, true, false, Narrow, true>(&win)
                                  : compactSearch<true, false, false, Narrow, true>(&win);
  CRes R;
  std::memcpy(&R, ldsMem.data() + oRes, sizeof(R));
  if (rc != R.status) return -3;
  out[0] = rc;
  out[1] = R.cost; out[2] = R.fmin; out[3] = R.nStates; out[4] = R.expanded; out[5] = R.nodes;
  out[6] = (int64_t)win.oobReads;
  out[7] = (int64_t)win.oobWrites;
  out[8] = tableInLds ? 1 : 0;
  out[9] = (int64_t)std::count_if(outPath.begin(), outPath.end(), [](uint16_t v) { return v != 0xBEEF; });
  if (rc == C_OK)
    for (int k = 0; k < R.nStates && k < states_cap; ++k) {
      states_xy[2 * k] = outPath[k] & 0xFF;
      states_xy[2 * k + 1] = outPath[k] >> 8;
    }
  return 0;
}

}  // extern "C"
