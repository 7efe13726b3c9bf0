// TEST INFRASTRUCTURE — wave_emu.h plus the two names libmultirobotplanning_amd/csrc/heur_bfs.h adds to the wave
// vocabulary (wave_dev.h): a lane permute and a masked halfword store into the LDS window.
#pragma once
#include "wave_emu.h"

namespace wv {

WV_FN V bpermute(const V& v, const V& src) {  // lane i receives lane src[i]'s value (ds_bpermute_b32)
  V r;
  for (int i = 0; i < kLanes; ++i) r.l[i] = v.l[src.l[i] & 63u];
  return r;
}
WV_FN void ldsStoreU16m(Lds l, const V& addr, const V& val, const B& m) {
  for (int i = 0; i < kLanes; ++i)
    if (((m.m >> i) & 1) && ldsIn(l, addr.l[i], 2, true)) {
      const uint16_t t = (uint16_t)val.l[i];
      memcpy(l->mem + addr.l[i], &t, 2);
    }
}

}  // namespace wv
