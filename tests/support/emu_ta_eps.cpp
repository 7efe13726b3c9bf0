// TEST INFRASTRUCTURE — one search of the LDS tier of MRP_LL_ASTAR_EPS_TA per call: ct::compactSearchTaEps
// (libmultirobotplanning_amd/csrc/ll_compact_ta_eps.h, the code the gfx950 kernels run) against the host interpretation of
// its wave vocabulary (wave_emu.h).  The job is put together as the engine does it: constraint words and the focal table by
// the host packer's own functions (csrc/host/ll_pack.h), the shortest-path table as mrp_ll_upload_heuristic lays it out
// ([32][32] halfwords, 0xFFFF unreachable), the window as the mixed kernels size it (4096 bytes behind ct::oPaths).
// Built by tests/test_eps_ta_tier_emu_cpu.py into tests/_build/libemu_ta_eps.so; never part of the product.
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <deque>
#include <vector>

//  45 decrease-key events (a_star_epsilon.hpp:254-269 taken)   46 ... that re-keyed a node sitting in the focal list
#define MRP_CT_COUNT_SLOTS 48
static int64_t g_te_counts[MRP_CT_COUNT_SLOTS];
#define MRP_CT_COUNT(k, v) (g_te_counts[k] += (int64_t)(v))

#include "wave_emu.h"
#include "../../libmultirobotplanning_amd/csrc/ll_compact_ta_eps.h"
#include "../../libmultirobotplanning_amd/csrc/host/ll_pack.h"

namespace {
struct Words {
  std::vector<uint32_t> w;
  bool failed = false;
  size_t size() const { return w.size(); }
  void push(uint32_t v) { w.push_back(v); }
};
}  // namespace

extern "C" {

enum { EMU_TE_NOT_TRIED = 100 };  // the job itself does not fit the tier (ct::taEpsJobFits): nothing was run

// obst_xy [n_obst][2]; has_goal = 0: an agent without a task; vc [n_vc][3] = t, x, y; ec [n_ec][5] = t, x1, y1, x2, y2;
// the focal context as the checker takes it: n_ctx paths, plen[a] states each, their x, y back to back in pxy, agent_idx's
// own entry ignored.  open_cap <= 1023, max_t <= 61, node_cap <= 1023: the tier's limits for this search.
// out[0..9] = status, cost, fmin, n_states, expanded, nodes, out-of-window LDS reads, writes, decrease-key events, those on
// a node in the focal list; cells[0 .. n_states) = x | y << 8.  Returns the status (== out[0]), EMU_TE_NOT_TRIED, or -2
// for an input out of range.
int emu_ta_eps_search(int dimx, int dimy, int n_obst, const int32_t* obst_xy, int sx, int sy, int has_goal, int gx, int gy,
                      int n_vc, const int32_t* vc, int n_ec, const int32_t* ec, float w, int agent_idx, int n_ctx,
                      const int32_t* plen, const int32_t* pxy, int64_t max_exp, int horizon, int open_cap, int max_t, int node_cap,
                      int64_t* out, int32_t* cells, int cells_cap) {
  using namespace mrp::ct;
  if (dimx < 1 || dimy < 1 || dimx > 255 || dimy > 255 || sx < 0 || sx >= dimx || sy < 0 || sy >= dimy) return -2;
  if (has_goal && (gx < 0 || gx >= dimx || gy < 0 || gy >= dimy)) return -2;
  if (open_cap < 6 || open_cap > (int)kCap || max_t < 0 || max_t > (int)kMaxT || node_cap < 6 || node_cap > (int)kTeNodeCap) return -2;
  const bool noGoal = !has_goal;
  Words cons;
  const int lastGoal = mrp::host::packVertexWords(vc, n_vc, dimx, dimy, horizon, gx, gy, noGoal, cons);
  const uint32_t nVc = (uint32_t)cons.size();
  mrp::host::packEdgeWords(ec, n_ec, dimx, dimy, horizon, cons);
  const uint32_t nEc = (uint32_t)cons.size() - nVc;
  cons.push(0);  // (never empty: the pointers below name something)
  std::vector<int32_t> len(plen, plen + n_ctx);
  std::vector<const int32_t*> xy((size_t)n_ctx);
  {
    size_t off = 0;
    for (int a = 0; a < n_ctx; ++a) {
      xy[a] = pxy + 2 * off;
      off += (size_t)len[a];
    }
  }
  const int tpad = n_ctx > 0 ? mrp::host::focalTableRows(n_ctx, agent_idx, len.data()) : 0;
  const uint32_t npad = tpad > 0 ? ((uint32_t)n_ctx + 15u) & ~15u : 0u;
  if (!taEpsJobFits((uint32_t)dimx, (uint32_t)dimy, nVc, nEc, npad)) return EMU_TE_NOT_TRIED;
  std::vector<uint16_t> table((size_t)tpad * npad + 1, 0xFFFFu);
  if (tpad > 0) mrp::host::fillFocalTable(table.data(), tpad, npad, n_ctx, agent_idx, len.data(), xy.data(), dimx, dimy);

  const uint32_t cellsN = (uint32_t)dimx * dimy;
  std::vector<uint32_t> obst((cellsN + 31) / 32, 0u);
  for (int i = 0; i < n_obst; ++i) {
    const int x = obst_xy[2 * i], y = obst_xy[2 * i + 1];
    if (x < 0 || x >= dimx || y < 0 || y >= dimy) continue;
    const uint32_t c = (uint32_t)(y * dimx + x);
    obst[c >> 5] |= 1u << (c & 31);
  }
  std::vector<uint16_t> heur(1024, 0xFFFFu);  // shortest_path_heuristic.hpp for the task's cell, [y * 32 + x]
  if (has_goal && !((obst[(gy * dimx + gx) >> 5] >> ((gy * dimx + gx) & 31)) & 1u)) {
    std::deque<int> q;
    heur[gy * 32 + gx] = 0;
    q.push_back(gy * 32 + gx);
    while (!q.empty()) {
      const int c = q.front();
      q.pop_front();
      const int x = c & 31, y = c >> 5;
      const int dxs[4] = {1, -1, 0, 0}, dys[4] = {0, 0, 1, -1};
      for (int k = 0; k < 4; ++k) {
        const int nx = x + dxs[k], ny = y + dys[k];
        if (nx < 0 || nx >= dimx || ny < 0 || ny >= dimy) continue;
        const uint32_t nc = (uint32_t)(ny * dimx + nx);
        if (((obst[nc >> 5] >> (nc & 31)) & 1u) || heur[ny * 32 + nx] != 0xFFFFu) continue;
        heur[ny * 32 + nx] = (uint16_t)(heur[c] + 1);
        q.push_back(ny * 32 + nx);
      }
    }
  }

  std::vector<uint8_t> ldsMem(oPaths + kTePathBytes, 0xA5);  // garbage from "the previous job"
  wv::LdsWindow win{ldsMem.data(), (uint32_t)ldsMem.size(), 0, 0};
  std::vector<uint8_t> parentTab(kParentBytes, 0xEE);
  std::vector<uint16_t> outPath(1024, 0);
  CJob J;
  std::memset(&J, 0, sizeof(J));
  J.dimx = dimx; J.dimy = dimy; J.sx = sx; J.sy = sy; J.gx = noGoal ? 0 : gx; J.gy = noGoal ? 0 : gy;
  J.lastGoal = lastGoal;
  J.w = w;
  J.nVc = nVc; J.nEc = nEc;
  J.vc = (uint64_t)(uintptr_t)cons.w.data(); J.ec = (uint64_t)(uintptr_t)(cons.w.data() + nVc);
  J.obst = (uint64_t)(uintptr_t)obst.data(); J.obstWords = (uint32_t)obst.size();
  J.nAgentsPad = npad; J.tPad = (uint32_t)tpad;
  J.pathsG = (uint64_t)(uintptr_t)table.data();
  J.bitsG = (uint64_t)(uintptr_t)heur.data();
  J.maxExp = max_exp < 0 ? 0xFFFFFFFFu : (uint32_t)std::min<int64_t>(max_exp, 0xFFFFFFFEll);
  J.openCap = (uint32_t)open_cap; J.maxT = (uint32_t)max_t; J.rows = (uint32_t)node_cap;
  J.taNoGoal = noGoal ? 1u : 0u;
  J.parentTab = (uint64_t)(uintptr_t)parentTab.data();
  J.outPath = (uint64_t)(uintptr_t)outPath.data();
  std::memcpy(ldsMem.data() + oJob, &J, sizeof(J));
  const int64_t dk0 = g_te_counts[45], dkf0 = g_te_counts[46];
  const int32_t rc = compactSearchTaEps(&win);
  CRes R;
  std::memcpy(&R, ldsMem.data() + oRes, sizeof(R));
  if (rc != R.status) return -3;
  out[0] = rc; out[1] = R.cost; out[2] = R.fmin; out[3] = R.nStates; out[4] = R.expanded; out[5] = R.nodes;
  out[6] = (int64_t)win.oobReads; out[7] = (int64_t)win.oobWrites;
  out[8] = g_te_counts[45] - dk0; out[9] = g_te_counts[46] - dkf0;
  if (rc == C_OK) {
    if (R.nStates < 1 || R.nStates > cells_cap) return -3;
    for (int k = 0; k < R.nStates; ++k) cells[k] = outPath[k];
  }
  return rc;
}

}  // extern "C"
