// Host check of the guard band and the image scale of the fp32-input MFMA sweeps (clustering_amd/csrc/dc_mfma32_band.hpp)
// for every chain length the sweeps are built for: S = 1..16 K-steps with both parities of D (D = 2 S - 1, 2 S).
//
// The chain is emulated in the order chains32 issues it -- float, fmaf, starting from the reference row's norm, two
// columns per step:  acc = |y'|^2;  acc = fmaf(y[2s+1], -2 x[2s+1], fmaf(y[2s], -2 x[2s], acc)),  s = 0 .. S-1  -- over
// random and adversarial vectors (all coordinates at the extent, alternating signs), and compared with the same
// quantity in long double:
//   1. unscaled (neighbour sweep):  |acc - (|y|^2 - 2 x.y)| <= guard_eps32(M, 4 M, 2 S, D)
//   2. scaled by c = scale32_pop(M, r^2, 2 S, D) (population sweep), threshold folded as the kernels fold it:
//      t = acc - ((fl(fl(c c) r^2) - 1) - |x''|^2)  against  c^2 (d^2 - r^2) + 1:  the error stays below 1, so the sign
//      (inside) and t >= 2 (outside) decide correctly and everything between goes to the exact re-check
//   3. scales 1e-12 .. 1e15 and r^2 in {0, tiny, M, 4 M, FLT_MAX}: c, c c and c c r^2 stay finite and c positive
// Exit status 0 and "OK" on success.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "dc_mfma32_band.hpp"

namespace {

int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      if (failures++ < 20) {        \
        printf("FAIL %s: ", #cond); \
        printf(__VA_ARGS__);        \
        printf("\n");               \
      }                             \
    }                               \
  } while (0)

struct Pair {
  std::vector<float> x, y;   // centred query / reference row, 2 S floats each (columns >= D zero)
};

long double norm2(const std::vector<float>& v) {
  long double s = 0;
  for (float f : v) s += (long double)f * f;
  return s;
}

float up(long double v) {   // a float not below v
  float f = (float)v;
  return ((long double)f < v) ? nextafterf(f, INFINITY) : f;
}

// the image pass: v = fl(c x) (c = 1: the value itself), norm = (float) of the double sum of squares
std::vector<float> image(const std::vector<float>& v, float c, bool scaled, float* norm) {
  std::vector<float> out(v.size());
  double n = 0.0;
  for (size_t k = 0; k < v.size(); ++k) {
    out[k] = scaled ? c * v[k] : v[k];
    n += (double)out[k] * (double)out[k];
  }
  *norm = (float)n;
  return out;
}

float chain(const std::vector<float>& xq, const std::vector<float>& yr, float norm_r, int S) {
  float acc = norm_r;
  for (int s = 0; s < S; ++s) {
    acc = fmaf(yr[2 * s], -2.0f * xq[2 * s], acc);
    acc = fmaf(yr[2 * s + 1], -2.0f * xq[2 * s + 1], acc);
  }
  return acc;
}

void check_pair(const Pair& p, int S, int D, const char* what) {
  const int K = 2 * S;
  const long double nx = norm2(p.x), ny = norm2(p.y);
  long double dot = 0, d2 = 0;
  for (size_t k = 0; k < p.x.size(); ++k) {
    dot += (long double)p.x[k] * p.y[k];
    const long double d = (long double)p.x[k] - p.y[k];
    d2 += d * d;
  }
  const float M = up(nx > ny ? nx : ny);
  if (!(M > 0.0f) || !(M <= 1.0e36f)) return;
  // 1. unscaled
  float nr = 0, nq = 0;
  const std::vector<float> yr = image(p.y, 1.0f, false, &nr), xq = image(p.x, 1.0f, false, &nq);
  const float acc = chain(xq, yr, nr, S);
  const long double err = fabsl((long double)acc - (ny - 2 * dot));
  const float eps = dc::guard_eps32(M, 4.0f * M, K, D);
  CHECK(err <= (long double)eps, "%s S=%d D=%d unscaled: error %Lg, band %g (M %g)", what, S, D, err, (double)eps, (double)M);
  // 2. scaled for r^2 = fl(d^2) of this very pair (the pair sits in the band: the hardest place), and for 4 M
  const float r2s[2] = {(float)d2, 4.0f * M};
  for (float r2 : r2s) {
    if (!(r2 <= FLT_MAX)) continue;
    if ((long double)r2 < d2 * 0.99L) continue;   // (the band is claimed for pairs up to the radius, not far beyond it)
    const float c = dc::scale32_pop(M, r2, K, D);
    float snr = 0, snq = 0;
    const std::vector<float> sy = image(p.y, c, true, &snr), sx = image(p.x, c, true, &snq);
    const float sacc = chain(sx, sy, snr, S);
    const float thr0 = (c * c) * r2 - 1.0f;
    const float thr = (thr0 > FLT_MAX) ? FLT_MAX : thr0;
    const float lo = thr - snq;
    const float t = sacc + (-lo);
    const long double want = (long double)c * c * (d2 - (long double)r2) + 1.0L;
    const long double terr = fabsl((long double)t - want);
    CHECK(terr < 1.0L, "%s S=%d D=%d scaled: error %Lg at c %g r2 %g (M %g, t %g, want %Lg)", what, S, D, terr, (double)c,
          (double)r2, (double)M, (double)t, want);
  }
}

void check_scales(int S, int D) {
  const int K = 2 * S;
  for (int e = -12; e <= 15; ++e) {
    const float ext = (float)pow(10.0, e);
    const float M = up((long double)D * ext * ext);
    const float r2s[5] = {0.0f, FLT_MIN, M, 4.0f * M, FLT_MAX};
    for (float r2max : r2s)
      for (float r2 : r2s) {
        if (r2 > r2max) continue;
        const float c = dc::scale32_pop(M, r2max, K, D);
        const float cc = c * c, ccr = cc * r2;
        CHECK(c > 0.0f && isfinite(c) && isfinite(cc) && cc > 0.0f && isfinite(ccr),
              "S=%d D=%d extent 1e%d r2max %g r2 %g: c %g, c c %g, c c r2 %g", S, D, e, (double)r2max, (double)r2, (double)c,
              (double)cc, (double)ccr);
      }
    const float cinf = dc::scale32_pop(M, INFINITY, K, D);
    CHECK(cinf == 0x1p-60f && isfinite(cinf * cinf * FLT_MAX), "S=%d D=%d: the lower clamp for r2max = +inf", S, D);
    CHECK(isfinite(dc::guard_eps32(M, 4.0f * M, K, D)) && dc::guard_eps32(M, 4.0f * M, K, D) > 0.0f, "S=%d D=%d: band", S, D);
  }
  CHECK(dc::scale32_pop(0.0f, 0.0f, K, D) == 0x1p63f, "S=%d D=%d: all rows equal, r = 0", S, D);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20260521);
  std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
  const float extents[] = {1.0e-12f, 3.0e-4f, 1.0f, 37.5f, 4096.0f, 1.0e15f};
  long pairs = 0;
  for (int S = 1; S <= 16; ++S)
    for (int D = 2 * S - 1; D <= 2 * S; ++D) {
      static_assert(dc::steps32(1) == 1 && dc::steps32(2) == 1 && dc::steps32(31) == 16 && dc::steps32(32) == 16, "K-steps");
      CHECK(dc::steps32(D) == S, "steps32(%d)", D);
      for (float ext : extents) {
        Pair p;
        p.x.assign(2 * S, 0.0f);
        p.y.assign(2 * S, 0.0f);
        // adversarial: all coordinates at the extent (same and opposite corners), alternating signs, one against the other
        for (int kind = 0; kind < 5; ++kind) {
          for (int k = 0; k < D; ++k) {
            const float alt = (k & 1) ? -ext : ext;
            p.x[k] = (kind == 0 || kind == 1) ? ext : alt;
            p.y[k] = (kind == 0) ? nextafterf(ext, 0.0f) : (kind == 1) ? -ext : (kind == 2) ? -alt : (kind == 3) ? nextafterf(alt, 0.0f) : ext;
          }
          check_pair(p, S, D, "adversarial");
          ++pairs;
        }
        for (int it = 0; it < 400; ++it) {
          for (int k = 0; k < D; ++k) {
            p.x[k] = ext * uni(rng);
            // (every fourth pair close together: cancellation in the Gram form)
            p.y[k] = (it % 4 == 0) ? p.x[k] * (1.0f + 1.0e-3f * uni(rng)) : ext * uni(rng);
          }
          check_pair(p, S, D, "random");
          ++pairs;
        }
      }
      check_scales(S, D);
    }
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("OK %ld pairs, S = 1..16, both parities of D\n", pairs);
  return 0;
}
