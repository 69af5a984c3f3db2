// Host check of the ring rule of the pruned wide neighbour sweep (clustering_amd/csrc/dc_wide_prune.hpp)
// against long-double arithmetic.  A query block meets a reference block in exactly one of three launches or never:
//   partition   for ANY bounds -- +inf, 0, equal, far2_hd below far2_nn, NaN-free free energies of any kind -- the classes
//               {seed, ring 1, ring 2, never} of wide_nn_ring are disjoint and cover every block (asked per launch, as the
//               kernel asks: "is this block in ring k?" is true for exactly one k of the four);
//   safety      G <= B_nn  =>  seed or ring 1 (a block that can hold a pair at or inside the bound is met with it);
//               G <= B_hd and fe_min(ref) < fe_max(query)  =>  met at all;
//   sharpness   G >= 1.0002 B_nn  =>  not ring 1;   G >= 1.0002 max(B_nn, B_hd)  =>  never, unless seed
//               (bounds at or above the smallest normal float: below it the rule keeps the floor);
//   the seed    is qb - 1, qb, qb + 1, whatever the gap and the bounds;
//   the floor   B = 0 (a block of duplicates) still meets the blocks at gap 0 and nothing with a positive normal gap.
// G is the real-number squared gap of the boxes.  Prints "ok <cases>" and returns 0, or the first violations and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>

#include "dc_wide_prune.hpp"

namespace {
const float kInf = std::numeric_limits<float>::infinity();
const float kFloor = std::numeric_limits<float>::min();
long cases = 0;
int failures = 0;

long double gap2_exact(const WideBox& a, const WideBox& b) {
  auto axis = [](long double alo, long double ahi, long double blo, long double bhi) {
    long double d = std::fmax(alo - bhi, blo - ahi);
    return d > 0.0L ? d : 0.0L;
  };
  if (a.lo0 > a.hi0 || b.lo0 > b.hi0 || a.lo1 > a.hi1 || b.lo1 > b.hi1) return std::numeric_limits<long double>::infinity();
  const long double dx = axis(a.lo0, a.hi0, b.lo0, b.hi0), dy = axis(a.lo1, a.hi1, b.lo1, b.hi1);
  return dx * dx + dy * dy;
}

struct Case {
  WideBox q, r;
  unsigned qb, rb;
  float b_nn, b_hd, fe_min_r, fe_max_q;
};

void fail(const char* what, const Case& c, int ring) {
  ++failures;
  if (failures <= 10)
    std::printf("FAIL %s: qb=%u rb=%u gap2=%a B_nn=%a B_hd=%a fe_min=%a fe_max=%a -> ring %d\n", what, c.qb, c.rb,
                wide_box_gap2(c.q, c.r), c.b_nn, c.b_hd, c.fe_min_r, c.fe_max_q, ring);
}

void check(const Case& c) {
  ++cases;
  const long double G = gap2_exact(c.q, c.r);
  const bool seed = wide_nn_is_seed(c.qb, c.rb);
  const float gap2 = wide_box_gap2(c.q, c.r), f_nn = wide_nn_far2(c.b_nn), f_hd = wide_nn_far2(c.b_hd);
  const int ring = wide_nn_ring(seed, gap2, f_nn, f_hd, c.fe_min_r, c.fe_max_q);
  // the partition, asked the way the three launches ask
  int hits = 0;
  for (int k = kWideRingSeed; k <= kWideRingNever; ++k) hits += wide_nn_ring(seed, gap2, f_nn, f_hd, c.fe_min_r, c.fe_max_q) == k;
  if (hits != 1 || ring < kWideRingSeed || ring > kWideRingNever) fail("not exactly one class", c, ring);
  const bool by_index = (long)c.rb >= (long)c.qb - 1 && (long)c.rb <= (long)c.qb + 1;
  if (seed != by_index || (ring == kWideRingSeed) != by_index) fail("the seed is qb - 1, qb, qb + 1", c, ring);
  if (seed) return;
  const bool fe_ok = c.fe_min_r < c.fe_max_q;
  if (std::isfinite((double)G)) {
    if (G <= (long double)c.b_nn && ring != kWideRing1) fail("a block at or inside the nn bound is not in ring 1", c, ring);
    if (G <= (long double)c.b_hd && fe_ok && ring == kWideRingNever) fail("a block inside the hd bound with a lower row is never met", c, ring);
  } else if (ring != kWideRingNever) {
    fail("an empty box is infinitely far", c, ring);
  }
  if (!fe_ok && ring == kWideRing2) fail("ring 2 holds a block without a lower row", c, ring);
  if (c.b_nn >= kFloor && std::isfinite(c.b_nn) && G >= 1.0002L * (long double)c.b_nn && ring == kWideRing1) fail("beyond the nn margin in ring 1", c, ring);
  const float b_max = std::fmax(c.b_nn, c.b_hd);
  if (b_max >= kFloor && std::isfinite(b_max) && G >= 1.0002L * (long double)b_max && ring != kWideRingNever) fail("beyond both margins and met", c, ring);
  if (ring == kWideRing2 && gap2 < f_nn) fail("ring 2 holds a block of ring 1", c, ring);
}
}  // namespace

int main() {
  const WideBox o{0.0f, 0.0f, 0.0f, 0.0f};
  const WideBox empty{kInf, -kInf, kInf, -kInf};
  const float bounds[] = {0.0f, 1e-45f, 1e-39f, kFloor, 1e-30f, 0.25f, 9.0f, 9.0f * 1.0001f, 1e12f, 3e38f, kInf};
  const float fes[] = {-kInf, -3e38f, -1.0f, -0.0f, 0.0f, 1e-45f, 1.25f, 3e38f, kInf};
  const float gaps[] = {0.0f, 1e-30f, 1e-19f, 0.5f, 3.0f, std::nextafter(3.0f, 0.0f), std::nextafter(3.0f, 4.0f), 3.0001f, 1e6f, 1e19f};
  for (float b_nn : bounds)
    for (float b_hd : bounds)
      for (float fe_min : fes)
        for (float fe_max : fes)
          for (float g : gaps)
            for (unsigned rb : {0u, 4u, 5u, 6u, 7u, 100u}) {
              check(Case{o, WideBox{g, g + 1.0f, 0.0f, 0.0f}, 5u, rb, b_nn, b_hd, fe_min, fe_max});
              check(Case{o, WideBox{0.6f * g, 0.6f * g, -0.8f * g - 2.0f, -0.8f * g}, 5u, rb, b_nn, b_hd, fe_min, fe_max});
            }
  for (float b : bounds) {
    check(Case{o, empty, 5u, 9u, b, b, 0.0f, 1.0f});
    check(Case{empty, o, 5u, 9u, b, kInf, 0.0f, 1.0f});
    check(Case{o, o, 0u, 0u, b, b, 0.0f, 0.0f});
    check(Case{o, o, 0u, 1u, b, b, 0.0f, 0.0f});
    check(Case{o, o, 0xFFFFFFFEu, 0xFFFFFFFFu, b, b, 0.0f, 0.0f});
  }
  // the floor: a block of duplicates (B = 0) meets the blocks at gap 0 and none at a positive normal gap
  if (wide_nn_ring(false, 0.0f, wide_nn_far2(0.0f), wide_nn_far2(0.0f), 0.0f, 0.0f) != kWideRing1) ++failures, std::printf("FAIL the floor keeps gap 0\n");
  if (wide_nn_ring(false, 1e-30f, wide_nn_far2(0.0f), wide_nn_far2(0.0f), 0.0f, 1.0f) != kWideRingNever) ++failures, std::printf("FAIL the floor keeps a positive gap\n");
  // +inf and equal bounds
  if (wide_nn_ring(false, 1e30f, wide_nn_far2(kInf), wide_nn_far2(kInf), 0.0f, 0.0f) != kWideRing1) ++failures, std::printf("FAIL an open bound meets every block with a row\n");
  if (wide_nn_ring(false, 9.0f, wide_nn_far2(4.0f), wide_nn_far2(4.0f), 0.0f, 1.0f) != kWideRingNever) ++failures, std::printf("FAIL equal bounds: ring 2 is empty\n");
  if (wide_nn_ring(false, 9.0f, wide_nn_far2(4.0f), wide_nn_far2(kInf), 1.0f, 1.0f) != kWideRingNever) ++failures, std::printf("FAIL fe_min == fe_max: no lower row\n");
  if (wide_nn_ring(false, 9.0f, wide_nn_far2(4.0f), wide_nn_far2(kInf), -0.0f, 0.0f) != kWideRingNever) ++failures, std::printf("FAIL -0 is not below +0\n");
  if (wide_nn_ring(false, 9.0f, wide_nn_far2(4.0f), wide_nn_far2(kInf), -kInf, kInf) != kWideRing2) ++failures, std::printf("FAIL -inf lies below +inf\n");
  cases += 7;
  // a random sweep: boxes at any magnitude, the bounds drawn around the gap
  std::mt19937_64 rng(20241);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int it = 0; it < 400000; ++it) {
    const double mag = std::ldexp(1.0, (int)(u(rng) * 40.0) - 20);
    auto box = [&]() {
      const float x = (float)((u(rng) - 0.5) * 8.0 * mag), y = (float)((u(rng) - 0.5) * 8.0 * mag);
      const float w = (float)(u(rng) * mag), h = (float)(u(rng) * mag);
      return WideBox{x, x + w, y, y + h};
    };
    Case c{box(), box(), (unsigned)(u(rng) * 50.0), (unsigned)(u(rng) * 50.0), 0.0f, 0.0f, (float)(u(rng) - 0.5), (float)(u(rng) - 0.5)};
    const long double G = gap2_exact(c.q, c.r);
    const double f[] = {0.5, 0.9999, 1.0, 1.00005, 1.0001, 1.00015, 1.0002, 2.0};
    c.b_nn = (float)((double)G / f[it & 7]);
    c.b_hd = (float)((double)G / f[(it >> 3) & 7]);
    check(c);
  }
  if (failures) {
    std::printf("%d failures in %ld cases\n", failures, cases);
    return 1;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
