// TEST INFRASTRUCTURE ONLY — the truth for MRP_LL_JOB_TABLE_H (include/mrp_ll.h): the oracle's AStar / AStarEpsilon
// (oracle/search_restated.hpp) over the oracle's grid Environment (oracle/mapf_restated.hpp: example/ecbs.cpp:247-522) with
// ONE thing replaced — admissibleHeuristic reads a table the caller passes in (a plain BFS of the test's, never the
// device's), as example/cbs.cpp:445-557 would with its switched-off shortest-path code.
//
// Built two ways by tests/table_h_checker.py: as a shared library for ctypes, and — with -DTABLE_H_CHECK_MAIN and
// -fsanitize=address,undefined — as a stand-alone program that reads cases from a text file and prints their results.
#include <stdint.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "mapf_restated.hpp"

using namespace oracle;
using namespace oracle::mapf;

namespace {

struct TableEnv {  // everything is the Environment's, except admissibleHeuristic
  Environment& env;
  const std::vector<Plan>& ctx;
  const int32_t* table;  // [dimy][dimx]; INT32_MAX: unreachable
  int dimx;
  int64_t cap;
  int admissibleHeuristic(const State& s) { return table[s.y * dimx + s.x]; }
  int focalStateHeuristic(const State& s, int g) { return env.focalStateHeuristic(s, g, ctx); }
  int focalTransitionHeuristic(const State& a, const State& b, int ga, int gb) { return env.focalTransitionHeuristic(a, b, ga, gb, ctx); }
  bool isSolution(const State& s) { return env.isSolution(s); }
  void getNeighbors(const State& s, std::vector<Neighbor<State, Action, int>>& n) { env.getNeighbors(s, n); }
  void onExpandNode(const State& s, int f, int g) {
    env.onExpandLowLevelNode(s, f, g);
    if (cap >= 0 && env.lowLevelExpanded() > cap) throw CapExceeded();
  }
  void onDiscover(const State&, int, int) {}
};

int actionCode(Action a) { return static_cast<int>(a); }  // ecbs.cpp:49-55: Up, Down, Left, Right, Wait = 0 .. 4

}  // namespace

extern "C" {

// algo 0 = AStar (with initialCost), 1 = AStarEpsilon (w).  ctxLen[nCtx] / ctxXY: the solution vector the focal heuristics
// see, as oracle_ll_search takes it.  out[0..3] = success, cost, fmin, n_states; statesTXY [cap][3]; actions [cap].
// Returns 0, or -1 when capExpansions was exceeded.  A start whose table value is INT32_MAX cannot reach the goal: the
// engine answers "no solution, nothing expanded" (mrp_ll.h), and so does this — g + INT_MAX is no f the reference could use.
int table_h_ll_search(int algo, float w, int dimx, int dimy, int nObst, const int32_t* obstXY, int agentIdx, int startX,
                      int startY, int goalX, int goalY, const int32_t* table, int nVC, const int32_t* vc, int nEC,
                      const int32_t* ec, int nCtx, const int32_t* ctxLen, const int32_t* ctxXY, int64_t capExpansions,
                      int initialCost, int32_t* out, int64_t* expanded, int32_t* statesTXY, int32_t* actions, int cap) {
  out[0] = out[1] = out[2] = out[3] = 0;
  *expanded = 0;
  if (table[startY * dimx + startX] == INT32_MAX) return 0;
  const int nGoals = std::max(nCtx, agentIdx + 1);
  std::vector<Cell> goals(static_cast<size_t>(nGoals), Cell{0, 0});
  goals[agentIdx] = Cell{goalX, goalY};
  std::unordered_set<Cell, CellHash> obstacles;
  for (int i = 0; i < nObst; ++i) obstacles.insert(Cell{obstXY[2 * i], obstXY[2 * i + 1]});
  Environment env(dimx, dimy, obstacles, goals);
  Constraints cons;
  for (int i = 0; i < nVC; ++i) cons.vertex.insert(VertexConstraint{vc[3 * i], vc[3 * i + 1], vc[3 * i + 2]});
  for (int i = 0; i < nEC; ++i) cons.edge.insert(EdgeConstraint{ec[5 * i], ec[5 * i + 1], ec[5 * i + 2], ec[5 * i + 3], ec[5 * i + 4]});
  std::vector<Plan> ctx(static_cast<size_t>(nCtx));
  int64_t off = 0;
  for (int a = 0; a < nCtx; ++a) {
    for (int k = 0; k < ctxLen[a]; ++k, ++off) ctx[a].states.push_back(std::make_pair(State(k, ctxXY[2 * off], ctxXY[2 * off + 1]), k));
    ctx[a].cost = ctxLen[a] ? ctxLen[a] - 1 : 0;
    ctx[a].fmin = 0;
  }
  env.setLowLevelContext(static_cast<size_t>(agentIdx), &cons);
  TableEnv shell{env, ctx, table, dimx, capExpansions};
  Plan plan;
  bool ok = false;
  int rc = 0;
  try {
    if (algo == 0) {
      AStar<State, Action, int, TableEnv, StateHash> ll(shell);
      ok = ll.search(State(0, startX, startY), plan, initialCost);
    } else {
      AStarEpsilon<State, Action, int, TableEnv, StateHash> ll(shell, w);
      ok = ll.search(State(0, startX, startY), plan);
    }
  } catch (const CapExceeded&) {
    rc = -1;
  }
  *expanded = env.lowLevelExpanded();
  const int n = ok ? static_cast<int>(plan.states.size()) : 0;
  out[0] = ok ? 1 : 0;
  out[1] = ok ? plan.cost : 0;
  out[2] = ok ? plan.fmin : 0;
  out[3] = n;
  for (int k = 0; k < n && k < cap; ++k) {
    statesTXY[3 * k + 0] = plan.states[k].first.time;
    statesTXY[3 * k + 1] = plan.states[k].first.x;
    statesTXY[3 * k + 2] = plan.states[k].first.y;
    if (k + 1 < n) actions[k] = actionCode(plan.actions[k].first);
  }
  return rc;
}

}  // extern "C"

#ifdef TABLE_H_CHECK_MAIN
// Stand-alone form: argv[1] is a text file of whitespace-separated integers (w as its binary32 bit pattern) —
//   nCases, then per case: algo wBits dimx dimy agentIdx sx sy gx gy cap initialCost nObst nVC nEC nCtx,
//   obst[nObst][2], table[dimy * dimx], vc[nVC][3], ec[nEC][5], ctxLen[nCtx], ctxXY[sum][2]
// One line per case on stdout: rc success cost fmin n_states expanded, then the states' t x y and the actions.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  auto rd = [&]() {
    long long v = 0;
    if (std::fscanf(f, "%lld", &v) != 1) {
      std::fprintf(stderr, "short case file\n");
      std::exit(2);
    }
    return v;
  };
  const int nCases = static_cast<int>(rd());
  for (int c = 0; c < nCases; ++c) {
    const int algo = static_cast<int>(rd());
    const uint32_t wBits = static_cast<uint32_t>(rd());
    float w;
    static_assert(sizeof(w) == sizeof(wBits), "binary32");
    std::memcpy(&w, &wBits, sizeof(w));
    const int dimx = static_cast<int>(rd()), dimy = static_cast<int>(rd()), agentIdx = static_cast<int>(rd());
    const int sx = static_cast<int>(rd()), sy = static_cast<int>(rd()), gx = static_cast<int>(rd()), gy = static_cast<int>(rd());
    const int64_t capExp = rd();
    const int initialCost = static_cast<int>(rd());
    const int nObst = static_cast<int>(rd()), nVC = static_cast<int>(rd()), nEC = static_cast<int>(rd()), nCtx = static_cast<int>(rd());
    auto block = [&](size_t n) {
      std::vector<int32_t> v(n + 1);  // (+ 1: data() of an empty list stays a valid pointer)
      for (size_t i = 0; i < n; ++i) v[i] = static_cast<int32_t>(rd());
      return v;
    };
    const std::vector<int32_t> obst = block(2 * static_cast<size_t>(nObst));
    const std::vector<int32_t> table = block(static_cast<size_t>(dimx) * dimy);
    const std::vector<int32_t> vc = block(3 * static_cast<size_t>(nVC)), ec = block(5 * static_cast<size_t>(nEC));
    const std::vector<int32_t> ctxLen = block(static_cast<size_t>(nCtx));
    size_t total = 0;
    for (int a = 0; a < nCtx; ++a) total += static_cast<size_t>(ctxLen[a]);
    const std::vector<int32_t> ctxXY = block(2 * total);
    const int cap = 2048;
    std::vector<int32_t> states(3 * cap), actions(cap);
    int32_t out[4];
    int64_t expanded = 0;
    const int rc = table_h_ll_search(algo, w, dimx, dimy, nObst, obst.data(), agentIdx, sx, sy, gx, gy, table.data(), nVC, vc.data(),
                                     nEC, ec.data(), nCtx, ctxLen.data(), ctxXY.data(), capExp, initialCost, out, &expanded,
                                     states.data(), actions.data(), cap);
    std::printf("%d %d %d %d %d %lld", rc, out[0], out[1], out[2], out[3], static_cast<long long>(expanded));
    for (int k = 0; k < out[3] && k < cap; ++k) std::printf(" %d %d %d", states[3 * k], states[3 * k + 1], states[3 * k + 2]);
    for (int k = 0; k + 1 < out[3] && k + 1 < cap; ++k) std::printf(" %d", actions[k]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
#endif
