// Host check of the seed rule of the pruned wide cross neighbour sweep (clustering_amd/csrc/dc_wide_prune.hpp
// wide_cross_seed_key) against long-double arithmetic.  The seed of a query block is the reference block of
// the least key (bits of c2) << 32 | block, c2 the float squared distance of the box centres in the plane:
//   nearest     the chosen block has a live row, and its real centre distance is the least of all live blocks' up to the
//               roundings of the float arithmetic (two centres, two differences, two squares, one sum);
//   unambiguous where the least and the second-least real distance differ by more than that rounding, the choice IS the
//               real-number argmin;
//   ties        equal boxes, equal centres (c2 = 0 for several blocks): the lowest block index wins;
//   no live row a block with lo > hi is never the seed while another block has a row; its key carries the high word ~0;
//   one block   is the seed whatever its box;
//   valid       whatever the boxes (NaN, inf, all empty), the seed is one of the blocks that were scanned;
//   partition   with the predicate rb == seed, the classes {seed, ring 1, ring 2, never} of wide_nn_ring are disjoint and
//               cover every block for ANY bounds, and the seed class is exactly the one block.
// Prints "ok <cases>" and returns 0, or the first violations and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "dc_wide_prune.hpp"

namespace {
const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();
const WideBox kEmpty{kInf, -kInf, kInf, -kInf};
long cases = 0;
int failures = 0;

// the reduction of wide_cross_seed_kernel: the least key over the blocks, its low word
unsigned seed_of(const WideBox& q, const std::vector<WideBox>& r) {
  unsigned long long best = ~0ull;
  for (unsigned b = 0; b < r.size(); ++b) {
    const unsigned long long k = wide_cross_seed_key(q, r[b], b);
    best = k < best ? k : best;
  }
  return (unsigned)best;
}

bool has_row(const WideBox& b) { return !(b.lo0 > b.hi0) && !(b.lo1 > b.hi1); }

// real centre distance and a bound on what the float arithmetic can add to or take from it (u = 2^-24 per operation)
void centre_distance(const WideBox& q, const WideBox& r, long double* c, long double* err) {
  const long double dx = 0.5L * ((long double)q.lo0 + q.hi0) - 0.5L * ((long double)r.lo0 + r.hi0);
  const long double dy = 0.5L * ((long double)q.lo1 + q.hi1) - 0.5L * ((long double)r.lo1 + r.hi1);
  *c = std::sqrt(dx * dx + dy * dy);
  const long double u = std::ldexp(1.0L, -24);
  const long double mag = std::fabs((long double)q.lo0) + std::fabs((long double)q.hi0) + std::fabs((long double)r.lo0) +
                          std::fabs((long double)r.hi0) + std::fabs((long double)q.lo1) + std::fabs((long double)q.hi1) +
                          std::fabs((long double)r.lo1) + std::fabs((long double)r.hi1);
  *err = 4.0L * u * mag + 8.0L * u * *c;
}

void fail(const char* what, unsigned seed, size_t n) {
  ++failures;
  if (failures <= 10) std::printf("FAIL %s: seed %u of %zu blocks\n", what, seed, n);
}

void check(const WideBox& q, const std::vector<WideBox>& r) {
  ++cases;
  const unsigned seed = seed_of(q, r);
  if (seed >= r.size()) return fail("the seed is no block of the reference", seed, r.size());
  bool any = false;
  for (const WideBox& b : r) any = any || has_row(b);
  if (!any) return;
  if (!has_row(r[seed])) return fail("the seed has no live row", seed, r.size());
  long double c_seed, e_seed;
  centre_distance(q, r[seed], &c_seed, &e_seed);
  if (!std::isfinite((double)c_seed)) return;   // (non-finite boxes: only validity is asked)
  for (unsigned b = 0; b < r.size(); ++b) {
    if (b == seed || !has_row(r[b])) continue;
    long double c, e;
    centre_distance(q, r[b], &c, &e);
    if (!std::isfinite((double)c)) continue;
    if (c + e + e_seed < c_seed) return fail("a block is nearer beyond the roundings", seed, r.size());
    const bool same = r[b].lo0 == r[seed].lo0 && r[b].hi0 == r[seed].hi0 && r[b].lo1 == r[seed].lo1 && r[b].hi1 == r[seed].hi1;
    if (same && b < seed) return fail("a tie went to the higher block", seed, r.size());
  }
}

void check_partition(unsigned seed, unsigned n_blocks, float gap2, float f_nn, float f_hd, float fe_min, float fe_max) {
  unsigned in_seed = 0;
  for (unsigned rb = 0; rb < n_blocks; ++rb) {
    ++cases;
    int hits = 0;
    for (int k = kWideRingSeed; k <= kWideRingNever; ++k)
      hits += wide_nn_ring(wide_cross_is_seed(seed, rb), gap2, f_nn, f_hd, fe_min, fe_max) == k;
    if (hits != 1) fail("not exactly one class", seed, n_blocks);
    const bool s = wide_nn_ring(wide_cross_is_seed(seed, rb), gap2, f_nn, f_hd, fe_min, fe_max) == kWideRingSeed;
    if (s != (rb == seed)) fail("the seed class is not the one block", seed, n_blocks);
    in_seed += s ? 1u : 0u;
  }
  if (in_seed != (seed < n_blocks ? 1u : 0u)) fail("the seed class holds another number of blocks than one", seed, n_blocks);
}
}  // namespace

int main() {
  const WideBox o{0.0f, 0.0f, 0.0f, 0.0f};
  // one block, whatever its box
  for (const WideBox& b : {o, WideBox{5.0f, 6.0f, -1.0f, 2.0f}, kEmpty, WideBox{kNaN, kNaN, 0.0f, 0.0f}, WideBox{kInf, kInf, 0.0f, 0.0f}}) {
    check(o, {b});
    if (seed_of(o, {b}) != 0u) fail("a single block is the seed", seed_of(o, {b}), 1);
  }
  // equal centres and equal boxes: the lowest index
  {
    const WideBox a{1.0f, 3.0f, 1.0f, 3.0f}, b{0.0f, 4.0f, 0.0f, 4.0f}, far{10.0f, 11.0f, 0.0f, 1.0f};
    const WideBox q{2.0f, 2.0f, 2.0f, 2.0f};
    struct { std::vector<WideBox> r; unsigned want; } const t[] = {
        {{far, a, b, a}, 1u}, {{b, a, far}, 0u}, {{far, far, far}, 0u}, {{kEmpty, far, far}, 1u}, {{kEmpty, kEmpty, a, kEmpty, b}, 2u},
        {{far, kEmpty, a}, 2u}, {{kEmpty, kEmpty}, 0u}};
    for (const auto& c : t) {
      check(q, c.r);
      if (seed_of(q, c.r) != c.want) fail("a tie or a block without a live row", seed_of(q, c.r), c.r.size());
    }
  }
  // the key: a block without a live row loses to any with one; the low word is the block; c2 orders the keys
  {
    ++cases;
    const WideBox q{0.0f, 2.0f, 0.0f, 2.0f};
    if ((wide_cross_seed_key(q, kEmpty, 7u) >> 32) != 0xFFFFFFFFull || (unsigned)wide_cross_seed_key(q, kEmpty, 7u) != 7u)
      fail("the key of a block without a live row", 7u, 0);
    if (wide_cross_seed_key(q, WideBox{3e38f, 3e38f, 3e38f, 3e38f}, 9u) >= wide_cross_seed_key(q, kEmpty, 0u))
      fail("an overflowing distance still beats a block without a live row", 9u, 0);
    if (wide_cross_seed_key(q, WideBox{1.0f, 1.0f, 1.0f, 1.0f}, 9u) != 9ull) fail("c2 = 0: the key is the block", 9u, 0);
    if (wide_cross_seed_key(q, WideBox{1.0f, 2.0f, 1.0f, 1.0f}, 0u) >= wide_cross_seed_key(q, WideBox{1.0f, 3.0f, 1.0f, 1.0f}, 0u))
      fail("a nearer centre has the smaller key", 0u, 0);
  }
  // non-finite boxes: the seed stays a block that was scanned
  check(WideBox{kNaN, kNaN, kNaN, kNaN}, {o, o, kEmpty});
  check(o, {WideBox{kNaN, 1.0f, 0.0f, 1.0f}, WideBox{-kInf, kInf, 0.0f, 0.0f}, kEmpty});
  check(WideBox{-kInf, kInf, 0.0f, 0.0f}, {o, WideBox{1.0f, 2.0f, 3.0f, 4.0f}});
  // a random sweep: boxes at any magnitude, up to 70 blocks, some without a live row, some repeated
  std::mt19937_64 rng(4261);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int it = 0; it < 60000; ++it) {
    const double mag = std::ldexp(1.0, (int)(u(rng) * 35.0) - 15);
    auto box = [&]() {
      const float x = (float)((u(rng) - 0.5) * 8.0 * mag), y = (float)((u(rng) - 0.5) * 8.0 * mag);
      const float w = (float)(u(rng) * mag), h = (float)(u(rng) * mag);
      return WideBox{x, x + w, y, y + h};
    };
    const unsigned n = 1u + (unsigned)(u(rng) * 70.0);
    std::vector<WideBox> r(n);
    for (unsigned b = 0; b < n; ++b) {
      const double pick = u(rng);
      r[b] = (pick < 0.1) ? kEmpty : (pick < 0.2 && b > 0) ? r[(unsigned)(u(rng) * b)] : box();
    }
    const WideBox q = box();
    check(q, r);
    // ... and where the real distances are apart by more than the roundings, the choice is the real argmin
    long double best = std::numeric_limits<long double>::infinity(), second = best, e_best = 0.0L;
    unsigned arg = 0;
    for (unsigned b = 0; b < n; ++b) {
      if (!has_row(r[b])) continue;
      long double c, e;
      centre_distance(q, r[b], &c, &e);
      if (c < best) {
        second = best;
        best = c;
        e_best = e;
        arg = b;
      } else if (c < second) {
        second = c;
      }
    }
    if (std::isfinite((double)best) && second - best > 4.0L * e_best + 1e-5L * second) {
      ++cases;
      if (seed_of(q, r) != arg) fail("an unambiguous nearest block is not the seed", seed_of(q, r), n);
    }
  }
  // the partition with the new predicate
  const float bounds[] = {0.0f, 1e-39f, 1.17549435e-38f, 0.25f, 9.0f, 9.0f * 1.0001f, 3e38f, kInf};
  const float fes[] = {-kInf, -1.0f, -0.0f, 0.0f, 1.25f, kInf};
  const float gaps[] = {0.0f, 1e-30f, 3.0f, std::nextafter(9.0f, 0.0f), 9.0f, std::nextafter(9.0f, 10.0f), 1e19f, kInf};
  for (float b_nn : bounds)
    for (float b_hd : bounds)
      for (float fe_min : fes)
        for (float fe_max : fes)
          for (float g : gaps)
            for (unsigned seed : {0u, 3u, 6u})
              check_partition(seed, 7u, g, wide_nn_far2(b_nn), wide_nn_far2(b_hd), fe_min, fe_max);
  if (failures) {
    std::printf("%d failures in %ld cases\n", failures, cases);
    return 1;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
