// Host check of what the pruned sweeps of 257..1024 columns rest on (clustering_amd/csrc/dc_wide_prune.hpp),
// against long-double arithmetic.  u = 2^-24, tiny = 2^-149 (the spacing of the subnormal floats).
//   step (c)    the canonical float sum d2_c of D squared differences, in each of the three summation orders of the
//               library's builds (four lanes; eight lanes; eight lanes with fused multiply-adds), against the real d2:
//                   d2 (1 - u)^(D+2) - D tiny  <=  d2_c  <=  d2 (1 + u)^(D+2) + D tiny
//               over random rows of 257, 512 and 1024 columns, magnitudes 1e-3 .. 1e3 (every product normal: the tiny
//               terms are not needed there and the test does not grant them) and over differences whose squares underflow;
//   the order   d2_c >= the float gap of the pair's own columns 0 / 1 (wide_box_gap2 of the two points): a float sum of
//               non-negative terms never falls below a partial sum of it, in any of the three orders;
//   the chain   for a bound X, a block pair that the rule drops (gap2 >= far2) holds only pairs with
//                   d2_c >= ((far2 - 2 tiny) / (1 + u)^4) (1 - u)^(D+2) - D tiny,
//               and this must be ABOVE X: for far2 = wide_nn_far2(B, wide_nn_floor(D)), X = max(B, floor), and for
//               far2 = wide_prune_far2(t, wide_pop_floor(D)), X = t, at every D of 257..1024;
//   the old floor  the floor argument of §4.24 written out -- 1.0001 (1 - u) / (1 + 2.4e-7) (1 - u)^(D+1) FLT_MIN
//               (1 - D tiny / FLT_MIN) -- is above FLT_MIN at 256 columns and BELOW the float under FLT_MIN at 1024: a
//               bound B just under FLT_MIN is a case it leaves open there;
//   the rule    wide_nn_ring under the floor of these widths at B = 0, B just under and just over the floor, with
//               subnormal and small gaps: decided as long-double arithmetic decides G against max(B, floor).
// Prints "ok <cases>" and returns 0, or the first violations and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "dc_wide_prune.hpp"

namespace {
const long double kU = 0x1p-24L, kTiny = 0x1p-149L, kFltMin = 0x1p-126L;
const float kFltMinF = std::numeric_limits<float>::min();
long cases = 0;
int failures = 0;

void fail(const char* what, int D, long double a, long double b) {
  ++failures;
  if (failures <= 12) std::printf("FAIL %s: D=%d %.12Le vs %.12Le\n", what, D, a, b);
}

// ---- the three canonical orders (dc_common.hpp), restated for the host ------------------------------------------------
float canon_sse2(const float* x, const float* y, int D) {
  auto sq = [&](int k) {
    const float c = x[k] - y[k];
    return c * c;
  };
  const int V = 4 * (D / 4);
  float a0 = sq(0), a1 = sq(1), a2 = sq(2), a3 = sq(3);
  for (int k0 = 4; k0 < V; k0 += 4) {
    a0 = a0 + sq(k0 + 0);
    a1 = a1 + sq(k0 + 1);
    a2 = a2 + sq(k0 + 2);
    a3 = a3 + sq(k0 + 3);
  }
  float s = (a0 + a2) + (a1 + a3);
  int k = V;
  if (D - k >= 2) {
    s = s + (sq(k) + sq(k + 1));
    k += 2;
  }
  if (D - k == 1) s = s + sq(k);
  return s;
}
template <bool FMA>
float canon_avx(const float* x, const float* y, int D) {
  auto df = [&](int k) { return x[k] - y[k]; };
  auto sq = [&](int k) {
    const float c = df(k);
    return c * c;
  };
  auto acc = [](float a, float c) { return FMA ? __builtin_fmaf(c, c, a) : a + c * c; };
  float s = 0.0f;
  int k = 0;
  const int V8 = 8 * (D / 8);
  float a[8];
  for (int l = 0; l < 8; ++l) a[l] = sq(l);
  for (int k0 = 8; k0 < V8; k0 += 8)
    for (int l = 0; l < 8; ++l) a[l] = acc(a[l], df(k0 + l));
  const float b0 = a[0] + a[4], b1 = a[1] + a[5], b2 = a[2] + a[6], b3 = a[3] + a[7];
  s = (b0 + b2) + (b1 + b3);
  k = V8;
  if (D - k >= 4) {
    const float t = (sq(k) + sq(k + 2)) + (sq(k + 1) + sq(k + 3));
    s = s + t;
    k += 4;
  }
  for (; k < D; ++k) s = acc(s, df(k));
  return s;
}

long double exact_d2(const float* x, const float* y, int D) {
  long double s = 0.0L;
  for (int k = 0; k < D; ++k) {
    const long double c = (long double)x[k] - (long double)y[k];
    s += c * c;
  }
  return s;
}

void check_sum(const float* x, const float* y, int D, bool normal) {
  const long double d2 = exact_d2(x, y, D);
  const long double lo = d2 * std::pow(1.0L - kU, D + 2) - (normal ? 0.0L : D * kTiny);
  const long double hi = d2 * std::pow(1.0L + kU, D + 2) + (normal ? 0.0L : D * kTiny);
  const WideBox px{x[0], x[0], x[1], x[1]}, py{y[0], y[0], y[1], y[1]};
  const float gap = wide_box_gap2(px, py);
  const float got[3] = {canon_sse2(x, y, D), canon_avx<false>(x, y, D), canon_avx<true>(x, y, D)};
  const char* names[3] = {"four lanes", "eight lanes", "eight lanes, fused"};
  for (int o = 0; o < 3; ++o) {
    ++cases;
    if ((long double)got[o] < lo * (1.0L - 1e-15L)) fail(names[o], D, got[o], lo);
    if ((long double)got[o] > hi * (1.0L + 1e-15L)) fail(names[o], D, got[o], hi);
    if (got[o] < gap) fail("the sum fell below the gap of its own columns 0 / 1", D, got[o], gap);
  }
}

// the least canonical sum a pair of a dropped block pair can have, by steps (b) and (c) with their absolute terms
long double chain_floor(float far2, int D) {
  const long double G = ((long double)far2 - 2.0L * kTiny) / std::pow(1.0L + kU, 4);
  return G * std::pow(1.0L - kU, D + 2) - D * kTiny;
}
}  // namespace

int main() {
  std::mt19937_64 rng(20251);
  std::uniform_real_distribution<double> uni(-1.0, 1.0), mag(-3.0, 3.0);
  // ---- step (c) and the order argument ----
  for (int D : {257, 512, 1024}) {
    std::vector<float> x(D), y(D);
    for (int rep = 0; rep < 400; ++rep) {
      const double scale = std::pow(10.0, mag(rng));   // 1e-3 .. 1e3
      for (int k = 0; k < D; ++k) {
        x[k] = (float)(scale * uni(rng));
        y[k] = (float)(scale * uni(rng));
      }
      check_sum(x.data(), y.data(), D, true);
      // ... a pair that differs in few columns, and a pair of duplicates but for columns 0 / 1
      for (int k = 8; k < D; ++k) y[k] = x[k];
      check_sum(x.data(), y.data(), D, true);
    }
    for (int rep = 0; rep < 400; ++rep) {   // squares around and below the subnormal range
      const double scale = std::pow(10.0, -19.0 - 3.5 * std::fabs(uni(rng)));
      for (int k = 0; k < D; ++k) {
        x[k] = (float)(scale * uni(rng));
        y[k] = (float)(scale * uni(rng));
      }
      check_sum(x.data(), y.data(), D, false);
    }
    // every other column loses its whole square: differences of 0.99 x 2^-75 square to 0.98 x 2^-150, which rounds to zero
    for (int k = 0; k < D; ++k) x[k] = 0.0f, y[k] = 0.99f * 0x1p-75f;
    y[0] = 0x1.01p-63f;   // column 0 alone carries a little more than FLT_MIN
    y[1] = 0.0f;
    check_sum(x.data(), y.data(), D, false);
    if (canon_sse2(x.data(), y.data(), D) != y[0] * y[0]) fail("the lost squares are not lost", D, canon_sse2(x.data(), y.data(), D), y[0] * y[0]);
  }

  // ---- the chain above its bound, under the floors of the width ----
  const float F = wide_nn_floor(1024);
  for (int D : {257, 300, 400, 401, 512, 1000, 1023, 1024}) {
    const float fl_nn = wide_nn_floor((unsigned)D), fl_pop = wide_pop_floor((unsigned)D);
    if (!(fl_nn == F && fl_pop == F && F >= kFltMinF)) fail("the floors of 257..1024 columns", D, fl_nn, fl_pop);
    const float bs[] = {0.0f, 0x1p-149f, std::nextafter(kFltMinF, 0.0f), kFltMinF, std::nextafter(F, 0.0f), F, std::nextafter(F, 1.0f),
                        2.0f * F, 1e-30f, 1e-6f, 1.0f, 9.0f, 1e30f};
    for (float B : bs) {
      ++cases;
      const float X = std::fmax(B, fl_nn);
      if (!(chain_floor(wide_nn_far2(B, fl_nn), D) > (long double)X)) fail("the neighbour chain ends at or below its bound", D, chain_floor(wide_nn_far2(B, fl_nn), D), X);
      if (B > 0.0f && !(chain_floor(wide_prune_far2(B, fl_pop), D) > (long double)B)) fail("the population chain ends at or below t", D, chain_floor(wide_prune_far2(B, fl_pop), D), B);
    }
    if (wide_prune_far2(0.0f, fl_pop) != 0.0f) fail("r2 = 0 keeps nothing at any floor", D, wide_prune_far2(0.0f, fl_pop), 0.0L);
  }
  // ... 65..256 columns keep their constants: FLT_MIN and no floor, the values of the one-argument calls
  for (unsigned D : {65u, 100u, 256u}) {
    ++cases;
    if (wide_nn_floor(D) != kFltMinF || wide_pop_floor(D) != 0.0f) fail("the floors of 65..256 columns", (int)D, wide_nn_floor(D), wide_pop_floor(D));
    for (float v : {0.0f, 1e-40f, 1e-38f, 0.5f, 9.0f, 1e30f, std::numeric_limits<float>::infinity()}) {
      if (wide_nn_far2(v, wide_nn_floor(D)) != wide_nn_far2(v)) fail("wide_nn_far2 moved", (int)D, wide_nn_far2(v, wide_nn_floor(D)), wide_nn_far2(v));
      if (wide_prune_far2(v, wide_pop_floor(D)) != wide_prune_far2(v) || wide_prune_far2(v) != 1.0001f * v)
        fail("wide_prune_far2 moved", (int)D, wide_prune_far2(v, wide_pop_floor(D)), 1.0001f * v);
    }
    if (!(chain_floor(wide_nn_far2(0.0f), (int)D) > kFltMin)) fail("the chain at FLT_MIN, 65..256 columns", (int)D, chain_floor(wide_nn_far2(0.0f), (int)D), kFltMin);
  }

  // ---- the old floor's argument, written out (§4.24 "The floor") ----
  auto old_written = [](int D) {
    return 1.0001L * (1.0L - kU) / (1.0L + 2.4e-7L) * std::pow(1.0L - kU, D + 1) * kFltMin * (1.0L - D * kTiny / kFltMin);
  };
  ++cases;
  if (!(old_written(256) > kFltMin)) fail("the old floor argument at 256 columns", 256, old_written(256), kFltMin);
  const float B_under = std::nextafter(kFltMinF, 0.0f);
  if (!(old_written(1024) < (long double)B_under)) fail("the old floor argument at 1024 columns is expected to fall short", 1024, old_written(1024), B_under);
  // the same case under the floor of the width: the chain closes, and the block at gap 2 FLT_MIN -- beyond the old bound,
  // inside the new one -- is met
  if (!(chain_floor(wide_nn_far2(B_under, F), 1024) > (long double)F)) fail("the new floor at 1024 columns", 1024, chain_floor(wide_nn_far2(B_under, F), 1024), F);
  if (wide_nn_ring(false, 2.0f * kFltMinF, wide_nn_far2(B_under, F), wide_nn_far2(B_under, F), 0.0f, 0.0f) != kWideRing1) fail("a gap of 2 FLT_MIN under the new floor", 1024, 0, 0);
  if (wide_nn_ring(false, 2.0f * kFltMinF, wide_nn_far2(B_under), wide_nn_far2(B_under), 0.0f, 0.0f) != kWideRingNever) fail("... and under the old one", 1024, 0, 0);

  // ---- the ring rule under the floor, against long-double arithmetic ----
  std::uniform_real_distribution<double> ex(-80.0, -55.0);
  const float bs[] = {0.0f, 0x1p-149f, 0x1p-130f, std::nextafter(F, 0.0f), F, std::nextafter(F, 1.0f), 1.5f * F, 4.0f * F};
  for (int rep = 0; rep < 20000; ++rep) {
    const float dx = rep % 7 == 0 ? 0.0f : (float)std::ldexp(1.0 + std::fabs(uni(rng)), (int)ex(rng));
    const float dy = rep % 5 == 0 ? 0.0f : (float)std::ldexp(1.0 + std::fabs(uni(rng)), (int)ex(rng));
    const WideBox q{-1.0f, 0.0f, -1.0f, 0.0f}, r{dx, dx + 1.0f, dy, dy + 1.0f};
    const long double G = (long double)dx * dx + (long double)dy * dy;
    const float gap2 = wide_box_gap2(q, r);
    if (std::fabs((long double)gap2 - G) > G * 4.0L * kU + 2.0L * kTiny) fail("the gap with subnormal squares", 0, gap2, G);
    for (float B : bs) {
      ++cases;
      const long double X = std::fmax(B, F);
      const float far2 = wide_nn_far2(B, F);
      const int ring = wide_nn_ring(false, gap2, far2, far2, 0.0f, 0.0f);
      if ((ring == kWideRing1) != (gap2 < far2)) fail("ring 1 is not gap2 < far2", 0, gap2, far2);
      if (G <= X && ring != kWideRing1) fail("a block at or inside the bound is not met", 0, G, X);
      if (G >= 1.0002L * X + 4.0L * kTiny && ring != kWideRingNever) fail("a block beyond the margin is met", 0, G, X);
    }
  }
  if (wide_nn_ring(false, 0.0f, wide_nn_far2(0.0f, F), wide_nn_far2(0.0f, F), 0.0f, 0.0f) != kWideRing1) fail("B = 0 keeps gap 0", 0, 0, 0);
  if (wide_nn_ring(false, 1e-30f, wide_nn_far2(0.0f, F), wide_nn_far2(0.0f, F), 0.0f, 1.0f) != kWideRingNever) fail("B = 0 keeps a gap of 1e-30", 0, 0, 0);

  if (failures) {
    std::printf("%d failures in %ld cases\n", failures, cases);
    return 1;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
