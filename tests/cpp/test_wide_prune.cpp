// Host check of the survivor rule of the pruned wide population sweep (clustering_amd/csrc/dc_wide_prune.hpp) against
// long-double arithmetic.  For boxes A, B and a threshold t = fl32(r^2) let G be the real-number squared gap of the boxes.
//   safety      G <= t               =>  the block survives (a pair inside the radius may lie on the boxes' nearest corners)
//   sharpness   G >= 1.0002 t        =>  it does not (the margin is 1.0001, its roundings a few 2^-24)
// and in between either answer is allowed -- except where the gap is EXACT in float (axis-aligned point pairs, the 3-4-5
// pairs): there the answer must be the long-double predicate G < 1.0001f x t itself, to the last float, which pins the
// margin constant (checked where the product 1.0001f x t is not within a rounding of G).  Cases: touching, overlapping, degenerate and empty boxes, gaps exactly at
// r^2, at 1.0001 r^2 and one float either side of both, r^2 = 0, r^2 = +inf, and a random sweep over magnitudes.
// Prints "ok <cases>" and returns 0, or the first violation and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "dc_wide_prune.hpp"

namespace {
const float kInf = std::numeric_limits<float>::infinity();
long cases = 0;
int failures = 0;

long double gap2_exact(const WideBox& a, const WideBox& b) {
  auto axis = [](long double alo, long double ahi, long double blo, long double bhi) {
    long double d = std::fmax(alo - bhi, blo - ahi);
    return d > 0.0L ? d : 0.0L;
  };
  const bool empty = a.lo0 > a.hi0 || b.lo0 > b.hi0 || a.lo1 > a.hi1 || b.lo1 > b.hi1;
  if (empty) return std::numeric_limits<long double>::infinity();
  const long double dx = axis(a.lo0, a.hi0, b.lo0, b.hi0), dy = axis(a.lo1, a.hi1, b.lo1, b.hi1);
  return dx * dx + dy * dy;
}

void fail(const char* what, const WideBox& a, const WideBox& b, float r2) {
  ++failures;
  if (failures <= 10)
    std::printf("FAIL %s: A=(%a,%a,%a,%a) B=(%a,%a,%a,%a) r2=%a gap2=%a far2=%a\n", what, a.lo0, a.hi0, a.lo1, a.hi1, b.lo0,
                b.hi0, b.lo1, b.hi1, r2, wide_box_gap2(a, b), wide_prune_far2(r2));
}

// the rule held to the real numbers, both ways round (the gap is symmetric)
void check(const WideBox& a, const WideBox& b, float r2) {
  ++cases;
  const long double G = gap2_exact(a, b);
  const float far2 = wide_prune_far2(r2);
  const bool s = wide_prune_survives(a, b, far2), s2 = wide_prune_survives(b, a, far2);
  if (s != s2) fail("asymmetric", a, b, r2);
  if (r2 > 0.0f && std::isfinite(G) && G <= (long double)r2 && !s) fail("a block that can hold a pair inside the radius was dropped", a, b, r2);
  if (std::isfinite(r2) && G >= 1.0002L * (long double)r2 && s) fail("a block beyond the margin survived", a, b, r2);
  if (r2 == 0.0f && s) fail("r2 = 0 keeps nothing", a, b, r2);
  if (std::isinf(G) && s) fail("an empty box is infinitely far", a, b, r2);
}

// the gap of (a, b) is exact in float: the answer is the real-number rule with the constant of the header, 1.0001f
void check_pinned(const WideBox& a, const WideBox& b, float r2) {
  check(a, b, r2);
  const long double G = gap2_exact(a, b), far = (long double)1.0001f * (long double)r2;
  if ((long double)wide_box_gap2(a, b) != G) {
    fail("the gap of this pair was to be exact in float", a, b, r2);
    return;
  }
  // fl(1.0001f r2) lies within 2^-24 of the product: a gap that close to it may fall on either side
  if (fabsl(G - far) <= far * 5.97e-8L) return;
  ++cases;
  if (wide_prune_survives(a, b, wide_prune_far2(r2)) != (G < far)) fail("the margin is not 1.0001f", a, b, r2);
}

float next(float x, int steps) {
  for (int k = 0; k < (steps < 0 ? -steps : steps); ++k) x = std::nextafter(x, steps < 0 ? -kInf : kInf);
  return x;
}
}  // namespace

int main() {
  const WideBox unit{0.0f, 1.0f, 0.0f, 1.0f};
  const WideBox empty{kInf, -kInf, kInf, -kInf};
  const float radii2[] = {0.0f, 1e-30f, 1e-6f, 0.25f, 1.0f, 9.0f, 3.078f, 1e12f, 3e38f, kInf};
  for (float r2 : radii2) {
    // touching (a shared edge, a shared corner), overlapping, one inside the other
    check(unit, WideBox{1.0f, 2.0f, 0.0f, 1.0f}, r2);
    check(unit, WideBox{1.0f, 2.0f, 1.0f, 2.0f}, r2);
    check(unit, WideBox{0.5f, 1.5f, -0.5f, 0.5f}, r2);
    check(unit, WideBox{0.25f, 0.75f, 0.25f, 0.75f}, r2);
    check(unit, unit, r2);
    // degenerate boxes: a point, a segment, two equal points
    check(WideBox{2.0f, 2.0f, 3.0f, 3.0f}, unit, r2);
    check(WideBox{2.0f, 2.0f, 3.0f, 3.0f}, WideBox{2.0f, 2.0f, 3.0f, 3.0f}, r2);
    check(WideBox{-1.0f, -1.0f, 0.0f, 5.0f}, WideBox{3.0f, 3.0f, 7.0f, 7.0f}, r2);
    // empty boxes on either side and on both
    check(unit, empty, r2);
    check(empty, unit, r2);
    check(empty, empty, r2);
  }
  // +inf keeps every pair of boxes that hold a row, 0 keeps none -- not even a block with itself
  if (!wide_prune_survives(unit, WideBox{1e19f, 1e19f, -1e19f, -1e19f}, wide_prune_far2(kInf))) fail("r2 = inf", unit, unit, kInf);
  if (wide_prune_survives(unit, unit, wide_prune_far2(0.0f))) fail("r2 = 0", unit, unit, 0.0f);
  // gaps exactly at r^2, at 1.0001 r^2, and a few floats either side: a point at the origin and a point at distance g
  // along one axis, and along the diagonal of a 3-4-5 triangle (both squares and their sum are exact)
  for (float r : {3.0f, 0.5f, 1.75f, 1024.0f, 3.0f * 1.52587890625e-05f}) {
    const float r2 = r * r;
    const WideBox o{0.0f, 0.0f, 0.0f, 0.0f};
    for (int st = -3; st <= 3; ++st) {
      const float g = next(r, st);
      check(o, WideBox{g, g, 0.0f, 0.0f}, r2);
      check(o, WideBox{-g - 7.0f, -g, 0.0f, 0.0f}, r2);
      check(o, WideBox{0.0f, 0.0f, g, g + 1.0f}, r2);
      const float far_edge = next((float)std::sqrt(1.0001 * (double)r2), st);
      check(o, WideBox{far_edge, far_edge, 0.0f, 0.0f}, r2);
      check(o, WideBox{0.6f * g, 0.6f * g, 0.8f * g, 0.8f * g}, r2);
    }
    // around the margin itself: the gap G = r^2 of these point pairs is exact in float, and the thresholds are the
    // floats either side of G / 1.0001f -- the answer flips where 1.0001f x t passes G, which pins the constant to 2^-23
    for (int st = -6; st <= 6; ++st) {
      const float t = next((float)((double)r2 / (double)1.0001f), st);
      check_pinned(o, WideBox{r, r, 0.0f, 0.0f}, t);
      check_pinned(WideBox{0.0f, 0.0f, -r, -r}, o, t);
      check_pinned(o, WideBox{0.6f * 5.0f, 0.6f * 5.0f, 4.0f, 4.0f}, next(25.0f / 1.0001f, st));
    }
    // the gap IS the radius: the nearest corners hold the pair one float inside, which must be met
    const WideBox inside{next(r, -1), 5.0f * r, -1.0f, 1.0f};
    if (!wide_prune_survives(WideBox{-r, 0.0f, -1.0f, 1.0f}, inside, wide_prune_far2(r2))) fail("one float inside", o, inside, r2);
    ++cases;
  }
  // a random sweep: boxes of any size at any magnitude, the threshold drawn around the gap
  std::mt19937_64 rng(20240);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int it = 0; it < 400000; ++it) {
    const double mag = std::ldexp(1.0, (int)(u(rng) * 40.0) - 20);
    auto box = [&]() {
      const float x = (float)((u(rng) - 0.5) * 8.0 * mag), y = (float)((u(rng) - 0.5) * 8.0 * mag);
      const float w = (float)(u(rng) * mag), h = (float)(u(rng) * mag);
      return WideBox{x, x + w, y, y + h};
    };
    const WideBox a = box(), b = box();
    const long double G = gap2_exact(a, b);
    const double f[] = {0.5, 0.9999, 1.0, 1.00005, 1.0001, 1.00015, 1.0002, 2.0};
    const float r2 = (float)((double)G / f[it & 7]);
    check(a, b, r2);
  }
  if (failures) {
    std::printf("%d failures in %ld cases\n", failures, cases);
    return 1;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
