// TEST INFRASTRUCTURE — stand-alone program (not wired into pytest): the searches of tests/push_cases.py through the emulator
// driver of emu_push.cpp in the three forms of the tier, for a run under the sanitizers:
//   python tests/push_cases.py /tmp/push_cases.txt
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -DMRP_CT_CHECK_TOPS -o /tmp/push_sanitize tests/support/push_sanitize_main.cpp && /tmp/push_sanitize /tmp/push_cases.txt
// The file holds, per case: name, dimx dimy, n_obst and the obstacles' x y, sx sy gx gy, n_vc and t x y each, n_ec and five
// numbers each, n_agents agent, the paths' lengths, their x y, and the oracle's status cost fmin n_states expanded.
// Exit status 0: every search gave the oracle's answer with no access outside the window (and, with -DMRP_CT_CHECK_TOPS, no
// disagreement of the kept heap roots).
#include "emu_push.cpp"

#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

static std::vector<int32_t> readN(std::istream& in, size_t n) {
  std::vector<int32_t> v(n);
  for (auto& x : v) in >> x;
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s CASES.txt\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string name;
  int bad = 0, n = 0;
  while (in >> name) {
    int dimx, dimy, nObst, sx, sy, gx, gy, nVc, nEc, nAgents, agent;
    in >> dimx >> dimy >> nObst;
    const std::vector<int32_t> obst = readN(in, 2 * (size_t)nObst);
    in >> sx >> sy >> gx >> gy >> nVc;
    const std::vector<int32_t> vc = readN(in, 3 * (size_t)nVc);
    in >> nEc;
    const std::vector<int32_t> ec = readN(in, 5 * (size_t)nEc);
    in >> nAgents >> agent;
    const std::vector<int32_t> plen = readN(in, (size_t)nAgents);
    size_t cells = 0;
    for (int32_t l : plen) cells += (size_t)l;
    const std::vector<int32_t> pxy = readN(in, 2 * cells);
    const std::vector<int32_t> want = readN(in, 5);
    if (!in) {
      std::fprintf(stderr, "%s: short file\n", name.c_str());
      return 2;
    }
    for (int form = 1; form <= 3; ++form) {
      int64_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      std::vector<int32_t> states(2 * 1024);
      const int rc = emu_compact_search(form, dimx, dimy, nObst, obst.data(), sx, sy, gx, gy, 1.3f, nVc, vc.data(), nEc, ec.data(),
                                        nAgents, agent, plen.data(), pxy.data(), -1, 0, 0, 0, out, states.data(), 1024);
      bool ok = rc == 0 && out[6] == 0 && out[7] == 0;
      for (int k = 0; k < 5; ++k) ok = ok && out[k] == want[k];
      n += 1;
      if (!ok) {
        bad += 1;
        std::printf("%s form %d: rc %d, got %ld %ld %ld %ld %ld (stray reads %ld writes %ld)\n", name.c_str(), form, rc, (long)out[0],
                    (long)out[1], (long)out[2], (long)out[3], (long)out[4], (long)out[6], (long)out[7]);
      }
    }
  }
  int64_t c[MRP_CT_COUNT_SLOTS];
  emu_push_counts(c, 0);
  std::printf("%d searches, %d wrong; kept roots checked %ld times, %ld disagreements\n", n, bad, (long)c[8], (long)c[9]);
  return bad != 0 || c[9] != 0 ? 1 : 0;
}
