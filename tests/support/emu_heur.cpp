// TEST INFRASTRUCTURE — the shortest-path table program (libmultirobotplanning_amd/csrc/heur_bfs.h, the code the gfx950
// kernel runs) compiled against the host interpretation of its wave vocabulary, one table per call.
// Built by tests/test_heuristic_emu_cpu.py into tests/_build/libemu_heur.so; never part of the product.
#include <stdint.h>

#include <vector>

#include "wave_emu_heur.h"
#include "../../libmultirobotplanning_amd/csrc/heur_bfs.h"

extern "C" {

// The bitmap is built exactly as mrp_ll_upload_map builds it (bit y * dimx + x, obstacles outside the grid ignored) and
// put, with the table behind it on a 32-word boundary, into one "maps buffer" with guard words around both; the LDS
// window has exactly the size the host asks the launch for.  dist[dimy][dimx] receives the table unpacked as
// mrp_ll_read_heuristic unpacks it (INT32_MAX = unreachable).
// out[0] = out-of-window LDS reads, out[1] = out-of-window LDS writes, out[2] = guard words changed, out[3] = LDS bytes.
int emu_heuristic_table(int dimx, int dimy, int n_obst, const int32_t* obst_xy, int gx, int gy, int32_t* dist, int64_t* out) {
  using namespace mrp::hb;
  if (dimx < 1 || dimy < 1 || dimx > 255 || dimy > 255 || gx < 0 || gx >= dimx || gy < 0 || gy >= dimy) return -2;
  const uint32_t cells = (uint32_t)dimx * dimy, mapWords = (cells + 31) / 32;
  const bool small = isSmall(dimx, dimy);
  const uint32_t tabWords = small ? 512u : (cells + 1) / 2;
  const uint32_t guard = 32, mapOff = guard, tabOff = (mapOff + mapWords + guard + 31u) & ~31u;
  const uint32_t kGuard = 0xA5A5A5A5u;
  std::vector<uint32_t> buf(tabOff + tabWords + guard, kGuard);
  for (uint32_t i = 0; i < mapWords; ++i) buf[mapOff + i] = 0;
  for (int i = 0; i < n_obst; ++i) {
    const int x = obst_xy[2 * i], y = obst_xy[2 * i + 1];
    if (x < 0 || x >= dimx || y < 0 || y >= dimy) continue;
    const uint32_t c = (uint32_t)(y * dimx + x);
    buf[mapOff + (c >> 5)] |= 1u << (c & 31);
  }
  const std::vector<uint32_t> before(buf);
  const uint32_t ldsSize = ldsBytes(dimx, dimy);
  std::vector<uint8_t> mem(ldsSize, 0xCD);
  wv::LdsWindow win{mem.data(), ldsSize, 0, 0};
  HeurJob job{mapOff, tabOff, (uint32_t)dimx | (uint32_t)dimy << 8, (uint32_t)gx | (uint32_t)gy << 8};
  heurBfs(&win, buf.data(), job);
  int64_t changed = 0;
  for (uint32_t i = 0; i < buf.size(); ++i)
    if ((i < tabOff || i >= tabOff + tabWords) && buf[i] != before[i]) ++changed;
  const uint16_t* t16 = reinterpret_cast<const uint16_t*>(buf.data() + tabOff);
  const int stride = small ? 32 : dimx;
  for (int y = 0; y < dimy; ++y)
    for (int x = 0; x < dimx; ++x) {
      const uint16_t v = t16[y * stride + x];
      dist[y * dimx + x] = v == 0xFFFFu ? INT32_MAX : (int32_t)v;
    }
  out[0] = (int64_t)win.oobReads;
  out[1] = (int64_t)win.oobWrites;
  out[2] = changed;
  out[3] = ldsSize;
  return 0;
}

}  // extern "C"
