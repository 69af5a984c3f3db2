// dc_mfma32_band.hpp -- the guard band and the image scale of the fp32-input MFMA sweeps (dc_mfma32.hpp), in a header
// that a host program can include on its own (tests/cpp/test_fp32_band.cpp checks both against long double arithmetic
// for every chain length the sweeps are built for).  No HIP header, no other header of the library.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DC_BAND32_HD __host__ __device__
#else
#define DC_BAND32_HD
#endif

namespace dc {

// (next_up of dc_mfma_kernels.hpp: f >= 0 finite; inf / NaN -> inf)
DC_BAND32_HD inline float band32_next_up(float f) {
  if (!(f <= FLT_MAX)) return INFINITY;
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + 1u);
}

// K-steps of a row of n_cols columns (two columns per v_mfma_f32_32x32x2_f32; an odd n_cols leaves the second half of
// its last step zero)
constexpr int steps32(int n_cols) { return (n_cols + 1) / 2; }

// band of the chain: eps = 1.25 u [(4 K + 10) M + (D / 4 + 12) d2cap], K = 2 S multiply-adds per chain, M = max |x'|^2
DC_BAND32_HD inline float guard_eps32(float M, float d2cap, int K, int D) {
  const double u = 5.9604644775390625e-8;
  const double cap = (d2cap > 0.0f) ? (double)d2cap : 0.0;
  return band32_next_up((float)(1.25 * u * ((4.0 * K + 10.0) * (double)M + (0.25 * D + 12.0) * cap)));
}

// scale c of the population image: the largest one at which the band of the scaled chain (see dc_mfma32.hpp) stays
// below 1 for squared radii up to r2max.  Every thread of the image pass and of the sweep evaluates this from the same
// words.
DC_BAND32_HD inline float scale32_pop(float M, float r2max, int K, int D) {
  const double u = 5.9604644775390625e-8;
  const double cap = (r2max > 0.0f) ? (double)r2max : 0.0;
  const double eps1 = 1.25 * u * ((4.0 * K + 13.0) * (double)M + (0.25 * D + 18.0) * cap);   // band at scale 1
  if (!(eps1 > 1.0e-76)) return 0x1p63f;                                                     // (all rows equal, r = 0)
  const float c = (float)(sqrt((1.0 - 1.0 / 65536.0) / eps1) * (1.0 - 1.0 / 1048576.0));
  // kept in [2^-60, 2^63] (a smaller c is always admissible: the band scales with S = c^2), so that S and S r2 stay finite
  // for every finite r2 -- at 2^64, S overflowed for data of spread ~1e-17 and every pair read as inside.  Only r2max =
  // +inf (a radius whose fl32 square overflows) takes the lower clamp; M <= 1e36 and finite r2 keep c above 2^-56.  In
  // such a launch chunk every finite radius gets thr ~ -1: all its pairs fall in the band and take the exact re-check
  // (pop32_fix), O(n^2) exact distances -- slow, and correct.
  return fminf(fmaxf(c, 0x1p-60f), 0x1p63f);
}

}  // namespace dc
