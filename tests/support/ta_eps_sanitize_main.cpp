// TEST INFRASTRUCTURE — stand-alone program: seeded searches through the emulator driver of emu_ta_eps.cpp (the LDS tier of
// MRP_LL_ASTAR_EPS_TA, csrc/ll_compact_ta_eps.h) for a run under the host sanitizers, which see what the emulator's window
// check does not: the tier's accesses to "device memory" — the cameFrom table, the focal path table, the heuristic table,
// the constraint words, the path out.  Built and run by tests/test_eps_ta_tier_sanitize_cpu.py:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o ta_eps_sanitize tests/support/ta_eps_sanitize_main.cpp && ./ta_eps_sanitize
// Maps of 4 .. 32 cells a side, with and without a task, constraints around start and goal and on the goal cell (late ones:
// free Waits, decrease-key events), contexts of 0 .. 128 random walks, w in {1.0, 1.3, 2.0}, small caps of every kind so
// that every exit of the search is taken.  Exit status 0: every search ended with a status of the tier's and no access
// outside its window; the counts printed say what was reached.
#include "emu_ta_eps.cpp"

#include <cstdio>
#include <vector>

namespace {
uint64_t g_seed = 20240917;
uint32_t rnd(uint32_t n) {  // [0, n)
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((g_seed >> 33) % n);
}
}  // namespace

int main() {
  int n = 0, bad = 0, byStatus[8] = {0, 0, 0, 0, 0, 0, 0, 0}, notTried = 0;
  int64_t dk = 0, rekeys = 0;
  for (int it = 0; it < 600; ++it) {
    const int dimx = 4 + (int)rnd(29), dimy = 4 + (int)rnd(29);
    std::vector<int32_t> obst;
    const int nObst = (int)rnd((uint32_t)(dimx * dimy / 5 + 1));
    for (int i = 0; i < nObst; ++i) {
      obst.push_back((int32_t)rnd((uint32_t)dimx));
      obst.push_back((int32_t)rnd((uint32_t)dimy));
    }
    obst.push_back(0); obst.push_back(0);  // (never empty; cell (0, 0) blocked)
    const int sx = 1 + (int)rnd((uint32_t)dimx - 1), sy = (int)rnd((uint32_t)dimy);
    const int gx = 1 + (int)rnd((uint32_t)dimx - 1), gy = (int)rnd((uint32_t)dimy);
    const int hasGoal = rnd(4) != 0;
    std::vector<int32_t> vc, ec;
    const int nVc = (int)rnd(12) + (rnd(10) == 0 ? 60 : 0);
    for (int i = 0; i < nVc; ++i) {
      const bool nearGoal = rnd(2) != 0;
      const int cx = nearGoal ? gx : sx, cy = nearGoal ? gy : sy;
      vc.push_back(1 + (int32_t)rnd(rnd(6) == 0 ? 70 : 14));
      vc.push_back(cx + (int32_t)rnd(3) - 1);
      vc.push_back(cy + (int32_t)rnd(3) - 1);
    }
    if (rnd(3) == 0) {  // a constraint on the goal (or, without a task, the start) cell itself
      vc.push_back(2 + (int32_t)rnd(40));
      vc.push_back(hasGoal ? gx : sx);
      vc.push_back(hasGoal ? gy : sy);
    }
    const int nEc = (int)rnd(8) + (rnd(12) == 0 ? 62 : 0);
    for (int i = 0; i < nEc; ++i) {
      const int x = sx + (int)rnd(5) - 2, y = sy + (int)rnd(5) - 2, d = (int)rnd(5);
      const int dxs[5] = {0, -1, 1, 0, 0}, dys[5] = {0, 0, 0, 1, -1};
      ec.push_back((int32_t)rnd(10)); ec.push_back(x); ec.push_back(y); ec.push_back(x + dxs[d]); ec.push_back(y + dys[d]);
    }
    vc.push_back(0); vc.push_back(0); vc.push_back(0);                       // (a constraint on a blocked cell: never matters)
    ec.push_back(0); ec.push_back(0); ec.push_back(0); ec.push_back(0); ec.push_back(0);
    const int nCtx = rnd(3) == 0 ? 0 : 1 + (int)rnd(rnd(8) == 0 ? 128 : 12);
    const int agent = nCtx ? (int)rnd((uint32_t)nCtx) : 0;
    std::vector<int32_t> plen, pxy;
    for (int a = 0; a < nCtx; ++a) {
      const int len = rnd(5) == 0 ? 0 : 1 + (int)rnd(40);
      plen.push_back(len);
      int x = sx + (int)rnd(7) - 3, y = sy + (int)rnd(7) - 3;
      for (int k = 0; k < len; ++k) {
        x = std::min(std::max(x + (int)rnd(3) - 1, 0), dimx - 1);
        y = std::min(std::max(y + (int)rnd(3) - 1, 0), dimy - 1);
        pxy.push_back(x); pxy.push_back(y);
      }
    }
    plen.push_back(0); pxy.push_back(0); pxy.push_back(0);
    const float ws[3] = {1.0f, 1.3f, 2.0f};
    const float w = ws[rnd(3)];
    const int64_t maxExp = rnd(6) == 0 ? (int64_t)rnd(200) : -1;
    const int openCap = rnd(5) == 0 ? 6 + (int)rnd(200) : 1023, maxT = rnd(5) == 0 ? (int)rnd(62) : 61;
    const int nodeCap = rnd(5) == 0 ? 6 + (int)rnd(300) : 1023;
    int64_t out[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int32_t cells[64];
    const int rc = emu_ta_eps_search(dimx, dimy, (int)obst.size() / 2, obst.data(), sx, sy, hasGoal, gx, gy, (int)vc.size() / 3, vc.data(),
                                     (int)ec.size() / 5, ec.data(), w, agent, nCtx, plen.data(), pxy.data(), maxExp, 1024, openCap, maxT,
                                     nodeCap, out, cells, 64);
    n += 1;
    if (rc == EMU_TE_NOT_TRIED) {
      notTried += 1;
      continue;
    }
    const bool known = rc == mrp::ct::C_OVERFLOW || (rc >= 0 && rc <= 5);
    if (!known || out[6] != 0 || out[7] != 0 || (rc == 0 && (out[3] < 1 || out[3] > 63))) {
      bad += 1;
      std::printf("search %d: rc %d, n_states %ld, stray reads %ld writes %ld\n", it, rc, (long)out[3], (long)out[6], (long)out[7]);
      continue;
    }
    byStatus[rc == mrp::ct::C_OVERFLOW ? 6 : rc] += 1;
    dk += out[8];
    rekeys += out[9];
  }
  std::printf("ta_eps_sanitize: %d searches, %d wrong, %d not tried; ok %d, no solution %d, cap %d, nodes %d, horizon %d, bad %d, "
              "focalH %d; decrease-key events %ld, in the focal list %ld\n",
              n, bad, notTried, byStatus[0], byStatus[1], byStatus[2], byStatus[3], byStatus[4], byStatus[5], byStatus[6], (long)dk,
              (long)rekeys);
  // what the seed was chosen to reach
  const bool reached = byStatus[0] >= 100 && byStatus[2] >= 5 && byStatus[3] >= 5 && byStatus[4] >= 5 && notTried >= 5 && dk >= 1;
  if (!reached) std::printf("ta_eps_sanitize: the seeded cases no longer reach what they are for\n");
  return bad != 0 || !reached ? 1 : 0;
}
