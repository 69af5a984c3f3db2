// The radial gap of the pruned neighbour sweep's ring rule.  For a frame x of a component with origin o
// let rho(x) = |(x - o)[2..D)|, the norm over the columns behind the two of the cell grid.  Columns 0/1 and the rest
// are orthogonal and rho is 1-Lipschitz in the rest, so for two frames of one component
//     d2(x, y) >= d2_01(x, y) + (rho(x) - rho(y))^2,
// and a tile that keeps the range [rho_lo, rho_hi] of its rows next to its box in columns 0/1 adds the squared distance
// of two intervals to the box gap.  Plain C++ that compiles for the device (order_rows2_kernel, nn_pruned_kernel) and
// for the host (tests/cpp/test_rho_gap.cpp draws interval pairs and holds the rounding rule to double arithmetic).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_RHO_FN __host__ __device__ __forceinline__
#else
#define DC_RHO_FN inline
#endif

// The stored range of a tile: lo / hi are the floats nearest to the smallest / largest rho of its rows (formed in
// double, so each is within half an ulp of the real number), widened outwards by 2^-21 of the larger end -- at least
// four of its ulps, and four ulps of lo all the more -- and by the smallest normal number, which covers ranges at the
// bottom of the exponent range.  The stored range contains the real-number rho of every float row of the tile.
// An empty range (+inf, -inf) stays what it is.
DC_RHO_FN void rho_range_widen(float& lo, float& hi) {
  const float w = hi * 4.76837158203125e-07f + 1.17549435e-38f;   // 2^-21 hi + FLT_MIN  (-inf for the empty range)
  if (lo <= hi) {
    lo = fmaxf(lo - w, 0.0f);
    hi = hi + w;
  }
}

// Squared distance of the stored ranges [a_lo, a_hi] and [b_lo, b_hi], rounded DOWN: never above (x - y)^2 for any
// reals x, y inside them.  The difference of two floats is rounded to nearest (at most 2^-24 too large), its square
// once more, so the product is below (1 + 2^-24)^3 of the real one; the factor 1 - 2^-20 takes sixteen times that
// off again.  A square below 2^-100 counts as no gap: towards the subnormals a rounding is no longer 2^-24 of the
// value.  (A gap whose square overflows gives +inf, as the distance itself would.)  An empty range on either side
// gives +inf (never inf - inf: the two differences pair +inf with -inf).
DC_RHO_FN float rho_gap2(float a_lo, float a_hi, float b_lo, float b_hi) {
  const float g = fmaxf(fmaxf(b_lo - a_hi, a_lo - b_hi), 0.0f);
  const float p = g * g;
  return (p >= 7.88860905e-31f) ? p * 0.99999904632568359375f : 0.0f;   // 2^-100; 1 - 2^-20
}
