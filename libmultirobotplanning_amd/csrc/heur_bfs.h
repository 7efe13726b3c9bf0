// Shortest-path heuristic tables as a wave program (vocabulary: wave_dev.h on the device, tests/support/wave_emu_heur.h on
// the host): ONE wavefront computes ONE table — ShortestPathHeuristic::getValue(cell, goal) of
// example/shortest_path_heuristic.hpp:12-63 for one goal cell, i.e. a 4-connected unit-weight BFS from the goal over the
// free cells of a map the engine already holds as a bitmap (bit y * dimx + x, mrp_ll_upload_map) — and leaves it in the
// layout the task-assignment searches read (mrp_ll_upload_heuristic): halfwords, 0xFFFF = unreachable,
//   maps up to 32 x 32 : [y * 32 + x], kHeurWords words      (bfsSmall: rows in registers, table image in LDS)
//   larger maps        : [y * dimx + x], (cells + 1) / 2 words (bfsLarge: bitmaps in LDS, distances straight to memory)
// The reference's graph has a vertex per cell and an edge between two adjacent cells when BOTH are free, and
// Floyd-Warshall's d[v][v] = 0 holds for every vertex: a goal on an obstacle gives 0 there and unreachable elsewhere.
// Control flow is wave-uniform (scalars from ballots only), as in ll_compact.h; integer work only, results are exact.
#pragma once
#include <stdint.h>

#include "heur_layout.h"

namespace mrp {
namespace hb {

using namespace wv;

// (HeurJob, kSmallLdsBytes, largeLdsBytes, isSmall: heur_layout.h, shared with the host)

// the lowest set bit of every lane's word (0 where the word is 0) and its index
WV_FN V lowBit(V v) { return v & (~v + splat(1u)); }
WV_FN V bitIndex(V low) { return popc(low - splat(1u)); }  // low != 0

// Maps up to 32 x 32.  Lane y holds row y of the map as one word each for "free and not reached yet" and "frontier"; one
// BFS step is  next = (f << 1 | f >> 1 | f[y - 1] | f[y + 1]) & avail  with the neighbouring rows through two lane
// permutes; the step number goes, one halfword per new bit, into a 2 KB LDS image of the table that leaves as 512
// coalesced words at the end.
WV_FN void bfsSmall(Lds l, uint32_t* maps, uint32_t mapOff, uint32_t tabOff, uint32_t dimx, uint32_t dimy, uint32_t gx,
                    uint32_t gy) {
  const V lane = laneId();
  const uint32_t nWords = (dimx * dimy + 31u) >> 5;
  for (uint32_t k = 0; k < 8u; ++k) ldsStore32(l, (lane + splat(64u * k)) << splat(2u), splat(0xFFFFFFFFu));
  // row y = bits y * dimx .. y * dimx + dimx - 1 of the bitmap: at most two words
  const B rowIn = lane < splat(dimy);
  const V bit0 = lane * splat(dimx);
  const V wi = bit0 >> splat(5u), sh = bit0 & splat(31u);
  const uint32_t* bm = maps + mapOff;
  const V lo = gLoad32m(bm, wi, rowIn & (wi < splat(nWords)));
  const V hi = gLoad32m(bm, wi + splat(1u), rowIn & (wi + splat(1u) < splat(nWords)));
  // (shift amounts are taken modulo 32: hi << (32 - 0) would be hi itself)
  const V obst = (lo >> sh) | sel(sh != splat(0u), hi << (splat(32u) - sh), splat(0u));
  const uint32_t rowMask = dimx == 32u ? 0xFFFFFFFFu : (1u << dimx) - 1u;
  V avail = sel(rowIn, ~obst & splat(rowMask), splat(0u));
  sync();
  const B goalRow = lane == splat(gy);
  ldsStoreU16m(l, ((lane << splat(5u)) + splat(gx)) << splat(1u), splat(0u), goalRow);  // d[goal][goal] = 0, obstacle or not
  V f = sel(goalRow, splat(1u << gx), splat(0u)) & avail;
  avail = avail & ~f;
  // lanes 32 .. 63 hold no row (avail = 0, f = 0): lane 0's "row above" (lane 63) and row 31's "row below" are empty
  const V up = (lane - splat(1u)) & splat(63u), dn = (lane + splat(1u)) & splat(63u);
  uint32_t step = 0;
  while (ballot(f != splat(0u)) != 0) {
    ++step;
    const V n = ((f << splat(1u)) | (f >> splat(1u)) | bpermute(f, up) | bpermute(f, dn)) & avail;
    avail = avail & ~n;
    V nb = n;
    while (ballot(nb != splat(0u)) != 0) {
      const V low = lowBit(nb);
      ldsStoreU16m(l, ((lane << splat(5u)) + bitIndex(low)) << splat(1u), splat(step), nb != splat(0u));
      nb = nb ^ low;
    }
    f = n;
  }
  sync();
  for (uint32_t k = 0; k < 8u; ++k) {
    const V idx = lane + splat(64u * k);
    gStore32m(maps + tabOff, idx, ldsLoad32(l, idx << splat(2u)), bsplat(true));
  }
}

// Larger maps (up to 255 x 255: 2033 words).  The bitmap stays in the engine's cell-linear form, bit c = y * dimx + x, so a
// step is four shifts of the whole frontier: by one bit each way (a move along x: bits that crossed a row boundary are
// taken out with the column-0 / last-column masks) and by dimx bits each way (a move along y).  "Available", the two
// frontiers and the two column masks live in LDS; the wave walks the words 64 at a time.  The table is filled with 0xFFFF
// first; every reached cell is then written once, straight to memory.
WV_FN void bfsLarge(Lds l, uint32_t* maps, uint32_t mapOff, uint32_t tabOff, uint32_t dimx, uint32_t dimy, uint32_t gx,
                    uint32_t gy) {
  const V lane = laneId();
  const uint32_t N = dimx * dimy, W = (N + 31u) >> 5, Wp = (W + 63u) & ~63u;
  const uint32_t oAvail = 0u, oCol0 = 4u * Wp, oColL = 8u * Wp;
  uint32_t oCur = 12u * Wp, oNxt = 16u * Wp;
  const uint32_t q = dimx >> 5, r = dimx & 31u;
  const uint32_t tabWords = (N + 1u) >> 1;
  uint16_t* tab = reinterpret_cast<uint16_t*>(maps + tabOff);
  const uint32_t* bm = maps + mapOff;
  const uint32_t tailMask = (1u << (N & 31u)) - 1u;  // the cells of word N / 32 (none when N is a multiple of 32)
  for (uint32_t c = 0; c < Wp; c += 64u) {
    const V i = lane + splat(c), a = i << splat(2u);
    const V obst = gLoad32m(bm, i, i < splat(W));
    const V valid = sel(i < splat(N >> 5), splat(0xFFFFFFFFu), sel(i == splat(N >> 5), splat(tailMask), splat(0u)));
    ldsStore32(l, a + splat(oAvail), ~obst & valid);
    ldsStore32(l, a + splat(oCol0), splat(0u));
    ldsStore32(l, a + splat(oColL), splat(0u));
    ldsStore32(l, a + splat(oCur), splat(0u));
    ldsStore32(l, a + splat(oNxt), splat(0u));
  }
  for (uint32_t c = 0; c < tabWords; c += 64u) {
    const V i = lane + splat(c);
    gStore32m(maps + tabOff, i, splat(0xFFFFFFFFu), i < splat(tabWords));
  }
  sync();
  for (uint32_t c = 0; c < dimy; c += 64u) {
    const V y = lane + splat(c);
    const B in = y < splat(dimy);
    const V c0 = y * splat(dimx), cl = c0 + splat(dimx - 1u);
    ldsOr32m(l, ((c0 >> splat(5u)) << splat(2u)) + splat(oCol0), splat(1u) << (c0 & splat(31u)), in);
    ldsOr32m(l, ((cl >> splat(5u)) << splat(2u)) + splat(oColL), splat(1u) << (cl & splat(31u)), in);
  }
  const uint32_t goalCell = gy * dimx + gx, gw = (goalCell >> 5) << 2;
  gStoreU16m(tab, splat(goalCell), splat(0u), lane == splat(0u));  // d[goal][goal] = 0, obstacle or not
  const uint32_t ga = ldsLoadS(l, oAvail + gw), fbit = (1u << (goalCell & 31u)) & ga;
  ldsStoreS(l, oAvail + gw, ga & ~fbit);
  ldsStoreS(l, oCur + gw, fbit);
  sync();
  bool any = fbit != 0u;
  uint32_t step = 0;
  while (any) {
    ++step;
    uint64_t found = 0;
    for (uint32_t c = 0; c < Wp; c += 64u) {
      const V i = lane + splat(c), a = i << splat(2u);
      const B in = i < splat(W);
      const V cur = splat(oCur);
      const V fc = ldsLoad32m(l, a + cur, in);
      // (i - 1, i - q, ... wrap far beyond W for the first words: the predicate keeps those lanes from loading)
      const V fm = ldsLoad32m(l, a - splat(4u) + cur, (i - splat(1u)) < splat(W));
      const V fp = ldsLoad32m(l, a + splat(4u) + cur, (i + splat(1u)) < splat(W));
      const V xp = ((fc << splat(1u)) | (fm >> splat(31u))) & ~ldsLoad32m(l, a + splat(oCol0), in);  // cell + 1
      const V xm = ((fc >> splat(1u)) | (fp << splat(31u))) & ~ldsLoad32m(l, a + splat(oColL), in);  // cell - 1
      const V a0 = ldsLoad32m(l, a - splat(4u * q) + cur, (i - splat(q)) < splat(W));
      const V b0 = ldsLoad32m(l, a + splat(4u * q) + cur, (i + splat(q)) < splat(W));
      V yp = a0, ym = b0;  // cell + dimx, cell - dimx
      if (r != 0u) {
        const V a1 = ldsLoad32m(l, a - splat(4u * q + 4u) + cur, (i - splat(q + 1u)) < splat(W));
        const V b1 = ldsLoad32m(l, a + splat(4u * q + 4u) + cur, (i + splat(q + 1u)) < splat(W));
        yp = (a0 << splat(r)) | (a1 >> splat(32u - r));
        ym = (b0 >> splat(r)) | (b1 << splat(32u - r));
      }
      const V av = ldsLoad32m(l, a + splat(oAvail), in);
      const V n = (xp | xm | yp | ym) & av;
      ldsStore32m(l, a + splat(oNxt), n, in);
      ldsStore32m(l, a + splat(oAvail), av & ~n, in);
      V nb = n;
      uint64_t left = ballot(nb != splat(0u));
      found |= left;
      while (left != 0) {
        const V low = lowBit(nb);
        gStoreU16m(tab, (i << splat(5u)) + bitIndex(low), splat(step), nb != splat(0u));
        nb = nb ^ low;
        left = ballot(nb != splat(0u));
      }
    }
    sync();
    const uint32_t t = oCur;
    oCur = oNxt;
    oNxt = t;
    any = found != 0;
  }
}

WV_ENTRY void heurBfs(Lds window, uint32_t* maps, const HeurJob job) {
  const Lds l = windowBase(window);
  const uint32_t dimx = job.dims & 255u, dimy = job.dims >> 8, gx = job.goal & 255u, gy = job.goal >> 8;
  if (isSmall(dimx, dimy))
    bfsSmall(l, maps, job.mapOff, job.tabOff, dimx, dimy, gx, gy);
  else
    bfsLarge(l, maps, job.mapOff, job.tabOff, dimx, dimy, gx, gy);
}

}  // namespace hb
}  // namespace mrp
