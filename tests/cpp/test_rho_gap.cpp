// Host check of the radial gap's rounding rule (clustering_amd/csrc/dc_rho_gap.hpp): the header's own
// rho_range_widen / rho_gap2 -- the text the kernels compile -- against double arithmetic.
//   contain  a stored range contains the real-number rho of every row it was formed from: doubles r, the floats nearest
//            to their minimum and maximum, widened
//   gap      for points x, y inside two stored ranges, rho_gap2 <= (x - y)^2 in double: the end points (the worst
//            case) and points in between, for ranges that overlap, touch, lie within a few ulps of each other or far
//            apart, at magnitudes from 1e-15 to 1e15 (squares inside the float range)
//   empty    an empty range stays empty and is infinitely far from everything, itself included (never NaN)
// usage: test_rho_gap <pairs>; prints "pairs <n> contain_failures <n> gap_failures <n> empty_failures <n> positive <n>"
// and OK when nothing failed.
#include "dc_rho_gap.hpp"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {   // splitmix64
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double uniform() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }
static float step_ulps(float x, int n) {
  for (int i = 0; i < abs(n); ++i) x = nextafterf(x, n > 0 ? INFINITY : 0.0f);
  return x;
}

int main(int argc, char** argv) {
  const long n_pairs = argc > 1 ? atol(argv[1]) : 1000000;
  long contain_failures = 0, gap_failures = 0, empty_failures = 0, positive = 0;
  for (long i = 0; i < n_pairs; ++i) {
    // magnitude: mostly that of real data, sometimes the ends of the exponent range
    const int kind = (int)(next_u64() % 8);
    const double mag = kind == 0 ? 1e-15 : kind == 1 ? 1e15 : kind == 2 ? 1e-3 : 1.0;
    // range a: from real numbers, as the ordering kernel forms it
    const double a0 = mag * uniform(), aw = mag * uniform() * (next_u64() % 2 ? 0.02 : 1e-7);
    const double a_min = a0, a_max = a0 + aw;
    float a_lo = (float)a_min, a_hi = (float)a_max;
    rho_range_widen(a_lo, a_hi);
    if (!((double)a_lo <= a_min && a_max <= (double)a_hi)) ++contain_failures;
    // range b: overlapping, starting within a few ulps of a's stored end, or well apart
    const int rel = (int)(next_u64() % 4);
    float b_lo, b_hi;
    if (rel == 0) {
      b_lo = step_ulps(a_hi, (int)(next_u64() % 9) - 2);          // -2 .. +6 ulps from touching
      b_hi = b_lo;
    } else if (rel == 1) {
      b_lo = (float)((double)a_hi * (1.0 + 1e-6 * uniform()));
      b_hi = b_lo;
    } else if (rel == 2) {
      b_lo = (float)(a_min + aw * uniform());                      // overlaps
      b_hi = b_lo;
    } else {
      b_lo = (float)((double)a_hi + mag * uniform());
      b_hi = b_lo;
    }
    b_hi = (float)((double)b_hi + mag * uniform() * 0.01);
    rho_range_widen(b_lo, b_hi);
    const bool swap = next_u64() % 2;
    const float g2 = swap ? rho_gap2(b_lo, b_hi, a_lo, a_hi) : rho_gap2(a_lo, a_hi, b_lo, b_hi);
    if (g2 > 0.0f) ++positive;
    const float xs[3] = {a_lo, a_hi, (float)((double)a_lo + ((double)a_hi - (double)a_lo) * uniform())};
    const float ys[3] = {b_lo, b_hi, (float)((double)b_lo + ((double)b_hi - (double)b_lo) * uniform())};
    for (float x : xs)
      for (float y : ys) {
        if (!(x >= a_lo && x <= a_hi && y >= b_lo && y <= b_hi)) continue;
        const double d = (double)x - (double)y;
        if (!((double)g2 <= d * d)) ++gap_failures;
      }
  }
  {
    float e_lo = INFINITY, e_hi = -INFINITY;
    rho_range_widen(e_lo, e_hi);
    if (!(e_lo == INFINITY && e_hi == -INFINITY)) ++empty_failures;
    if (!(rho_gap2(e_lo, e_hi, 0.1f, 0.2f) == INFINITY)) ++empty_failures;
    if (!(rho_gap2(0.1f, 0.2f, e_lo, e_hi) == INFINITY)) ++empty_failures;
    if (!(rho_gap2(e_lo, e_hi, e_lo, e_hi) == INFINITY)) ++empty_failures;
    if (!(rho_gap2(0.0f, 0.0f, 0.0f, 0.0f) == 0.0f)) ++empty_failures;   // (the ranges at two columns, or no ranges)
  }
  printf("pairs %ld contain_failures %ld gap_failures %ld empty_failures %ld positive %ld\n", n_pairs, contain_failures,
         gap_failures, empty_failures, positive);
  const bool ok = contain_failures == 0 && gap_failures == 0 && empty_failures == 0;
  if (ok) printf("OK\n");
  return ok ? 0 : 1;
}
