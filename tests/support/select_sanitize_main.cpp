// TEST INFRASTRUCTURE — stand-alone program (not wired into pytest): the searches of tests/loop_exit_cases.py and of
// tests/push_cases.py through the emulator driver of emu_select.cpp in the three forms of the tier, for a run under the
// sanitizers:
//   python tests/loop_exit_cases.py /tmp/loop_exit_cases.txt && python tests/push_cases.py /tmp/push_cases.txt
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o /tmp/select_sanitize tests/support/select_sanitize_main.cpp
//   /tmp/select_sanitize /tmp/loop_exit_cases.txt /tmp/push_cases.txt
// (and once more with -DMRP_CT_EXEC_STORES, -DMRP_CT_PLAIN_LOOP, -DMRP_CT_PLAIN_EXPANSION).
// The first file has the format tests/loop_exit_cases.py's dump describes, the second the one push_sanitize_main.cpp
// describes.  Exit status 0: every search gave what its case expects with no access outside the window.
#include "emu_select.cpp"

#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

static std::vector<int32_t> readN(std::istream& in, size_t n) {
  std::vector<int32_t> v(n);
  for (auto& x : v) in >> x;
  return v;
}

// knobs: the first file's six numbers in front of the oracle's words
static int runFile(const char* path, bool knobs, int& n) {
  std::ifstream in(path);
  std::string name;
  int bad = 0;
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
    std::vector<int32_t> k = {-1, 0, 0, 0, 0, 7};  // max_exp open_cap max_t kind code forms
    if (knobs) k = readN(in, 6);
    const std::vector<int32_t> want = readN(in, 5);
    if (!in) {
      std::fprintf(stderr, "%s: short file\n", name.c_str());
      return -1;
    }
    for (int form = 1; form <= 3; ++form) {
      if (!((k[5] >> (form - 1)) & 1)) continue;
      int64_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      std::vector<int32_t> states(2 * 1024);
      const int rc = emu_compact_search(form, dimx, dimy, nObst, obst.data(), sx, sy, gx, gy, 1.3f, nVc, vc.data(), nEc, ec.data(),
                                        nAgents, agent, plen.data(), pxy.data(), k[0], 0, k[1], k[2], out, states.data(), 1024);
      bool ok = rc == 0 && out[6] == 0 && out[7] == 0;
      if (k[3] == 0)
        for (int q = 0; q < 5; ++q) ok = ok && out[q] == want[q];
      else if (k[3] == 1)
        ok = ok && out[0] == 2 && out[4] == k[0] + 1;
      else
        ok = ok && out[0] == -1 && out[1] == k[4] && out[4] < want[4];
      n += 1;
      if (!ok) {
        bad += 1;
        std::printf("%s form %d: rc %d, got %ld %ld %ld %ld %ld (stray reads %ld writes %ld)\n", name.c_str(), form, rc, (long)out[0],
                    (long)out[1], (long)out[2], (long)out[3], (long)out[4], (long)out[6], (long)out[7]);
      }
    }
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s LOOP_EXIT_CASES.txt [PUSH_CASES.txt]\n", argv[0]);
    return 2;
  }
  int n = 0;
  const int bad1 = runFile(argv[1], true, n);
  const int bad2 = argc > 2 ? runFile(argv[2], false, n) : 0;
  if (bad1 < 0 || bad2 < 0) return 2;
  std::printf("%d searches, %d wrong\n", n, bad1 + bad2);
  return bad1 + bad2 != 0 ? 1 : 0;
}
