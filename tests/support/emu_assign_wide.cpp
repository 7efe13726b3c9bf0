// TEST INFRASTRUCTURE — the wide assignment wave program (libmultirobotplanning_amd/csrc/assign_wave_wide.h, the code the
// gfx950 kernel runs) compiled against the host interpretation of its wave vocabulary, behind the engine's own wide packer
// (host/assign_pack.h) and next-best series (host/assign_series.h).  A program of its own: built by
// tests/test_assign_wide_emu_cpu.py with the host sanitizers, it reads records from stdin and writes results to stdout.
//
//   budget B                                               (the LDS budget of the records that follow: the row source)
//   solve  nA nT minMatching hasMode maskWords  cost[nA*nT]  [mode[nA]]  [forbidden[nA][maskWords]]
//          (maskWords 0: no forbidden masks, mask_words = ceil(nT / 64))
//   sparse nA nT minMatching  nEdges [a t cost]*  nModes [a mode]*  nForbidden [a t]*    (no edge where none is given)
//   narrow nA nT minMatching hasMode hasForbidden  cost[nA*nT]  [mode[nA]]  [forbidden[nA]]   (the NARROW program)
//   gsolve dimx dimy nA nT maskWords  table[nT][dimy*dimx]  starts[nA][2]  allowed[nA][maskWords]
//   series nA nT cost[nA*nT]                                (the whole wide series, then two more calls)
// Every record answers with lines "R status matched cost task_of...", a series with "S <lines>" first; the last line is
// "OOB <reads> <writes>": the LDS accesses outside the window assign_layout.h computes.  Every staged area — the data
// words, the result area with its scratch regions, the LDS window — is a heap block of exactly its size, so
// AddressSanitizer sees an access past it.
#include <stdint.h>

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "wave_emu_assign.h"
#include "../../libmultirobotplanning_amd/csrc/assign_wave_wide.h"
#include "../../libmultirobotplanning_amd/csrc/host/assign_pack.h"
#include "../../libmultirobotplanning_amd/csrc/host/assign_series.h"

using namespace mrp::host;

namespace {

uint64_t g_oobReads = 0, g_oobWrites = 0;
uint32_t g_budget = mrp::as::kLdsBudgetWide;

// what mrp_ll_assign_batch_w does, with the emulator in the kernel's place
int solveBatchWide(const PackEnv& env, const std::vector<uint32_t>& maps, int32_t n, const mrp_ll_assign_problem_w* problems,
                   mrp_ll_assign_result* results) {
  AssignStagingWide st;
  packAssignBatchWide(env, n, problems, results, g_budget, st);
  std::vector<uint32_t> out(st.outWords + st.scratchWords, 0xA5A5A5A5u);
  const std::vector<uint32_t> data(st.data.begin(), st.data.end());  // (capacity = size)
  for (const mrp::as::AssignJobWide& job : st.jobs) {
    const uint32_t bytes = mrp::as::ldsBytesWide(job.nA, job.nT, g_budget);
    if (bytes > st.ldsBytes) return MRP_LL_E_INVALID;
    std::vector<uint8_t> mem(bytes, 0xCD);
    wv::LdsWindow win{mem.data(), bytes, 0, 0};
    mrp::as::assignSolveWideAny(&win, maps.data(), data.data(), out.data(), job);
    g_oobReads += win.oobReads;
    g_oobWrites += win.oobWrites;
  }
  unpackAssignBatchWide(st, out.data(), results);
  return MRP_LL_SUCCESS;
}

int solveBatchNarrow(int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results) {
  const PackEnv env;
  const std::vector<uint32_t> maps(1, 0);
  AssignStaging st;
  packAssignBatch(env, n, problems, results, st);
  std::vector<uint32_t> out(st.outWords, 0xA5A5A5A5u);
  for (const mrp::as::AssignJob& job : st.jobs) {
    std::vector<uint8_t> mem(st.ldsBytes, 0xCD);
    wv::LdsWindow win{mem.data(), mrp::as::ldsBytes(job.nA), 0, 0};
    mrp::as::assignSolve(&win, maps.data(), st.data.data(), out.data(), job);
    g_oobReads += win.oobReads;
    g_oobWrites += win.oobWrites;
  }
  unpackAssignBatch(st, out.data(), results);
  return MRP_LL_SUCCESS;
}

void printResult(const mrp_ll_assign_result& r, int nA) {
  std::printf("R %d %d %lld", r.status, r.matched, (long long)r.cost);
  for (int a = 0; a < nA; ++a) std::printf(" %d", r.task_of[a]);
  std::printf("\n");
}

template <class T>
std::vector<T> readN(size_t n) {
  std::vector<T> v(n);
  for (T& x : v) std::cin >> x;
  return v;
}

}  // namespace

int main() {
  std::string kind;
  const PackEnv noEnv;
  const std::vector<uint32_t> noMaps(1, 0);
  static const int32_t none = 0;
  while (std::cin >> kind) {
    if (kind == "budget") {
      std::cin >> g_budget;
    } else if (kind == "solve") {
      int nA, nT, minM, hasMode, mw;
      std::cin >> nA >> nT >> minM >> hasMode >> mw;
      const size_t rows = nA > 0 ? nA : 0, cols = nT > 0 ? nT : 0;
      const std::vector<int32_t> cost = readN<int32_t>(rows * cols);
      const std::vector<int32_t> mode = readN<int32_t>(hasMode ? rows : 0);
      const std::vector<uint64_t> forb = readN<uint64_t>(rows * (size_t)mw);
      std::vector<int32_t> taskOf(rows + 1, -7);
      mrp_ll_assign_problem_w p{nA, nT, cost.empty() ? &none : cost.data(), nullptr, nullptr, nullptr,
                                mw ? forb.data() : nullptr, hasMode ? mode.data() : nullptr, minM,
                                mw ? mw : std::max(1, (nT + 63) / 64)};
      mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
      solveBatchWide(noEnv, noMaps, 1, &p, &r);
      printResult(r, (int)std::min<size_t>(rows, 256));
    } else if (kind == "sparse") {
      int nA, nT, minM, nEdges, nModes, nForb;
      std::cin >> nA >> nT >> minM >> nEdges;
      const int mw = std::max(1, (nT + 63) / 64);
      std::vector<int32_t> cost((size_t)nA * nT, MRP_LL_ASSIGN_NO_EDGE), mode((size_t)nA, MRP_LL_ASSIGN_FREE);
      std::vector<uint64_t> forb((size_t)nA * mw, 0);
      for (int e = 0; e < nEdges; ++e) {
        int a, t, c;
        std::cin >> a >> t >> c;
        cost[(size_t)a * nT + t] = c;
      }
      std::cin >> nModes;
      for (int e = 0; e < nModes; ++e) {
        int a, m;
        std::cin >> a >> m;
        mode[a] = m;
      }
      std::cin >> nForb;
      for (int e = 0; e < nForb; ++e) {
        int a, t;
        std::cin >> a >> t;
        forb[(size_t)a * mw + t / 64] |= 1ull << (t % 64);
      }
      std::vector<int32_t> taskOf((size_t)nA + 1, -7);
      mrp_ll_assign_problem_w p{nA, nT, cost.empty() ? &none : cost.data(), nullptr, nullptr, nullptr, forb.data(), mode.data(), minM, mw};
      mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
      solveBatchWide(noEnv, noMaps, 1, &p, &r);
      printResult(r, nA);
    } else if (kind == "narrow") {
      int nA, nT, minM, hasMode, hasForb;
      std::cin >> nA >> nT >> minM >> hasMode >> hasForb;
      const size_t rows = nA > 0 ? nA : 0, cols = nT > 0 ? nT : 0;
      const std::vector<int32_t> cost = readN<int32_t>(rows * cols);
      const std::vector<int32_t> mode = readN<int32_t>(hasMode ? rows : 0);
      const std::vector<uint64_t> forb = readN<uint64_t>(hasForb ? rows : 0);
      std::vector<int32_t> taskOf(rows + 1, -7);
      mrp_ll_assign_problem p{nA, nT, cost.empty() ? &none : cost.data(), nullptr, nullptr, nullptr,
                              hasForb ? forb.data() : nullptr, hasMode ? mode.data() : nullptr, minM};
      mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
      solveBatchNarrow(1, &p, &r);
      printResult(r, (int)std::min<size_t>(rows, 64));
    } else if (kind == "gsolve") {
      int dimx, dimy, nA, nT, mw;
      std::cin >> dimx >> dimy >> nA >> nT >> mw;
      PackEnv env;
      env.maps.push_back(MapRec{dimx, dimy, (uint32_t)(dimx * dimy + 31) / 32, 0});
      const MapRec& mp = env.maps[0];
      std::vector<uint32_t> maps(32, 0xA5A5A5A5u);  // tables on their own 128-byte lines, exactly their words
      std::vector<int32_t> ids;
      for (int t = 0; t < nT; ++t) {
        const std::vector<int32_t> dist = readN<int32_t>((size_t)dimx * dimy);
        const uint32_t off = (uint32_t)maps.size();
        maps.resize(maps.size() + heurTableWords(mp), 0xFFFFFFFFu);
        uint16_t* t16 = reinterpret_cast<uint16_t*>(maps.data() + off);
        for (int y = 0; y < dimy; ++y)
          for (int x = 0; x < dimx; ++x) {
            const int32_t v = dist[y * dimx + x];
            t16[y * heurStride(mp) + x] = (v < 0 || v > 0xFFFE) ? 0xFFFFu : (uint16_t)v;
          }
        while (maps.size() & 31u) maps.push_back(0xA5A5A5A5u);
        env.heurs.push_back(HeurRec{0, off});
        ids.push_back(t);
      }
      const std::vector<int32_t> starts = readN<int32_t>(2 * (size_t)nA);
      const std::vector<uint64_t> allowed = readN<uint64_t>((size_t)nA * mw);
      std::vector<int32_t> taskOf((size_t)nA + 1, -7);
      mrp_ll_assign_problem_w p{nA, nT, nullptr, ids.data(), starts.data(), allowed.data(), nullptr, nullptr, 0, mw};
      mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
      const std::vector<uint32_t> exact(maps.begin(), maps.end());
      solveBatchWide(env, exact, 1, &p, &r);
      printResult(r, nA);
    } else if (kind == "series") {
      int nA, nT;
      std::cin >> nA >> nT;
      const std::vector<int32_t> cost = readN<int32_t>((size_t)nA * nT);
      mrp_ll_assign_problem_w p{nA, nT, cost.empty() ? &none : cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                std::max(1, (nT + 63) / 64)};
      const AssignSolveWideFn solveWide = [&](int32_t n, const mrp_ll_assign_problem_w* ps, mrp_ll_assign_result* rs) {
        return solveBatchWide(noEnv, noMaps, n, ps, rs);
      };
      const AssignSolveFn solve = [&](int32_t n, const mrp_ll_assign_problem* ps, mrp_ll_assign_result* rs) {
        return solveBatchNarrow(n, ps, rs);
      };
      mrp_ll_assign_series* s = nullptr;
      if (assignSeriesCreateWide(nullptr, 1, &p, &s, solveWide) != MRP_LL_SUCCESS) {
        std::printf("S 0\n");
        continue;
      }
      std::vector<std::string> lines;
      std::vector<int32_t> taskOf((size_t)nA + 1, -7);
      for (int after = 0; after < 3;) {
        mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
        if (assignSeriesNext(1, &s, &r, solve, solveWide) != MRP_LL_SUCCESS) break;
        if (r.status != MRP_LL_OK) ++after;  // exhausted: ask twice more
        std::string line = "R " + std::to_string(r.status) + " " + std::to_string(r.matched) + " " + std::to_string(r.cost);
        for (int a = 0; a < nA; ++a) line += " " + std::to_string(taskOf[a]);
        lines.push_back(line);
      }
      std::printf("S %zu\n", lines.size());
      for (const std::string& l : lines) std::printf("%s\n", l.c_str());
      delete s;
    } else {
      std::fprintf(stderr, "emu_assign_wide: unknown record \"%s\"\n", kind.c_str());
      return 2;
    }
  }
  std::printf("OOB %llu %llu\n", (unsigned long long)g_oobReads, (unsigned long long)g_oobWrites);
  return 0;
}
