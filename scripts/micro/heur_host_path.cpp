// Helper of scripts/heuristic_tables.py: the host's way to a set of shortest-path tables, as a C caller of the engine
// walks it — a queue BFS per goal cell, mrp_ll_upload_heuristic per table, one mrp_ll_sync_maps — timed piece by piece.
// Built by the script (g++ -O2, linked against libmrp_ll.so); not part of the product.
#include <stdint.h>

#include <chrono>
#include <climits>
#include <vector>

#include "mrp_ll.h"

extern "C" int heur_host_path(mrp_ll_ctx* ctx, int32_t map_id, int32_t dimx, int32_t dimy, int32_t n_obst,
                              const int32_t* obst_xy, int32_t n, const int32_t* goals_xy, int32_t* heuristic_ids,
                              double* ms /* [3]: BFS, upload, sync */) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const int32_t cells = dimx * dimy;
  std::vector<uint8_t> blocked(cells, 0);
  for (int32_t i = 0; i < n_obst; ++i) {
    const int32_t x = obst_xy[2 * i], y = obst_xy[2 * i + 1];
    if (x >= 0 && x < dimx && y >= 0 && y < dimy) blocked[y * dimx + x] = 1;
  }
  std::vector<int32_t> dist(cells), queue(cells);
  ms[0] = ms[1] = ms[2] = 0.0;
  for (int32_t k = 0; k < n; ++k) {
    auto t0 = clk::now();
    const int32_t g = goals_xy[2 * k + 1] * dimx + goals_xy[2 * k];
    for (int32_t c = 0; c < cells; ++c) dist[c] = INT32_MAX;
    dist[g] = 0;
    int32_t head = 0, tail = 0;
    if (!blocked[g]) queue[tail++] = g;
    while (head < tail) {
      const int32_t c = queue[head++], x = c % dimx, y = c / dimx, d = dist[c] + 1;
      if (x + 1 < dimx && !blocked[c + 1] && dist[c + 1] == INT32_MAX) dist[c + 1] = d, queue[tail++] = c + 1;
      if (x > 0 && !blocked[c - 1] && dist[c - 1] == INT32_MAX) dist[c - 1] = d, queue[tail++] = c - 1;
      if (y + 1 < dimy && !blocked[c + dimx] && dist[c + dimx] == INT32_MAX) dist[c + dimx] = d, queue[tail++] = c + dimx;
      if (y > 0 && !blocked[c - dimx] && dist[c - dimx] == INT32_MAX) dist[c - dimx] = d, queue[tail++] = c - dimx;
    }
    ms[0] += since(t0);
    t0 = clk::now();
    const int rc = mrp_ll_upload_heuristic(ctx, map_id, dist.data(), &heuristic_ids[k]);
    ms[1] += since(t0);
    if (rc != MRP_LL_SUCCESS) return rc;
  }
  auto t0 = clk::now();
  const int rc = mrp_ll_sync_maps(ctx);
  ms[2] = since(t0);
  return rc;
}
