// TEST INFRASTRUCTURE — wave_emu.h plus the two names libmultirobotplanning_amd/csrc/assign_wave.h adds to the wave
// vocabulary (wave_dev.h): a predicate made from a wave-uniform lane mask and the 64-lane unsigned minimum.
#pragma once
#include "wave_emu.h"

namespace wv {

WV_FN B laneMask(uint64_t m) { return B{m}; }
WV_FN uint32_t waveMinU32(const V& v) {
  uint32_t r = v.l[0];
  for (int i = 1; i < kLanes; ++i) r = v.l[i] < r ? v.l[i] : r;
  return r;
}

}  // namespace wv
