// The survivor rule of the pruned wide population sweep: which reference blocks a query block has to meet.
// Every block of 128 positions of the spatial order keeps the box of its rows in the (col 0, col 1) plane, the original
// floats; a reference block survives the scan of a query block iff
//     box_gap2(query box, reference box)  <  far2 = 1.0001f x (the largest fl32(r^2) of the launch),
// the rule of pop_pruned_kernel.  A pair of frames is at least as far apart as the boxes of its blocks, so a block that
// does not survive holds no pair inside any radius of the launch -- with the roundings of the gap and of the canonical
// sum of up to 256 columns inside the margin (the proof: DESIGN §4.22; up to 1024 columns: §4.33).
// Plain C++ that compiles for the device (wide_sweep_kernel's pruned form) and for the host
// (tests/cpp/test_wide_prune.cpp holds the rule to long-double arithmetic).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_PRUNE_FN __host__ __device__ __forceinline__
#else
#define DC_PRUNE_FN inline
#endif

// (lo0, hi0, lo1, hi1); no live row: (+inf, -inf, +inf, -inf), infinitely far from everything
struct WideBox {
  float lo0, hi0, lo1, hi1;
};

// squared distance of two boxes in the plane -- the one copy of this arithmetic: box_gap2 (dc_mfma_kernels.hpp), which
// every pruned sweep calls on its float4 boxes, is this function -- two float differences,
// their squares, one sum -- within 4 x 2^-24 of the real number.  An empty box on either side: +inf.
DC_PRUNE_FN float wide_box_gap2(const WideBox& a, const WideBox& b) {
  const float dx = fmaxf(0.0f, fmaxf(a.lo0 - b.hi0, b.lo0 - a.hi0));
  const float dy = fmaxf(0.0f, fmaxf(a.lo1 - b.hi1, b.lo1 - a.hi1));
  return dx * dx + dy * dy;
}

// The smallest bound the steps of the proofs are argued for.  A product that underflows -- a square of the
// gap, a square of the canonical sum -- loses up to 2^-149 absolutely, (D + 2) 2^-149 in all; against a bound X the chain
// of the proof then ends at X (1.0001 (1 - u) (1 + u)^-4 (1 - u)^(D+2) - (D + 2) 2^-149 / X), which is above X only for
// X > 0.37 FLT_MIN at 256 columns and X > 3.2 FLT_MIN at 1024.  Up to 256 columns the rules keep the constants they were
// written with (no floor for a radius, FLT_MIN for a neighbour bound); beyond, both take 16 FLT_MIN = 2^-122, where the
// chain ends at 1.00003 X at 1024 columns (tests/cpp/test_xwide_prune.cpp evaluates it in long doubles).
constexpr float kWidePruneFloorXWide = 1.8807909613156436e-37f;   // 2^-122, exact
DC_PRUNE_FN float wide_pop_floor(unsigned n_cols) { return n_cols <= 256u ? 0.0f : kWidePruneFloorXWide; }
DC_PRUNE_FN float wide_nn_floor(unsigned n_cols) { return n_cols <= 256u ? 1.17549435e-38f : kWidePruneFloorXWide; }

// r2max: the largest fl32(r^2) of the launch (a number >= 0 or +inf; a NaN radius came in as 0).  floor: wide_pop_floor
// of the width -- a positive radius below it prunes as the floor does (r2max = 0 keeps nothing at any floor)
DC_PRUNE_FN float wide_prune_far2(float r2max, float floor = 0.0f) { return 1.0001f * (r2max > 0.0f ? fmaxf(r2max, floor) : r2max); }
// ... as every launcher of a pruned population sweep forms it, self and cross: under the floor of the launch's width
DC_PRUNE_FN float wide_prune_far2_at(float r2max, unsigned n_cols) { return wide_prune_far2(r2max, wide_pop_floor(n_cols)); }

// The factor of wide_nn_start (dc_mfma_wide_kernels.hpp) for (1 - u)^-(D+2), u = 2^-24: the real d2 of a row is at most its
// canonical float sum times this, in whatever order the sum is formed.  1 + 2.0e-5 holds up to 256 columns
// (the term is 1.54e-5 there); at 512 columns the term is 3.06e-5, at 1024 6.12e-5, and both pruned neighbour instances,
// self and cross, take 1 + 7.0e-5 beyond 256 columns (tests/cpp/test_xwide_cross_prune.cpp holds the premise to long doubles).
constexpr float kWideNnGrow = 1.0f + 2.0e-5f, kXWideNnGrow = 1.0f + 7.0e-5f;
DC_PRUNE_FN float wide_nn_grow(unsigned n_cols) { return n_cols <= 256u ? kWideNnGrow : kXWideNnGrow; }

// r2 = 0 keeps nothing (no pair has d2 < 0), r2 = +inf every block with a live row
DC_PRUNE_FN bool wide_prune_survives(const WideBox& query, const WideBox& ref, float far2) {
  return wide_box_gap2(query, ref) < far2;
}

// ---- the rings of the pruned wide neighbour sweep --------------------------------------------------------
// A query block meets its reference blocks in three launches, and the three sets partition the blocks it meets:
//   seed    the blocks qb - 1, qb, qb + 1 of the order (those there are): no bound is known yet;
//   ring 1  the other blocks with gap2 < far2_nn, the bound of the block's nearest neighbours after the seed;
//   ring 2  the blocks of neither with gap2 < far2_hd, the bound of its nearest neighbours of lower free energy after
//           ring 1, that hold a row of lower free energy than some query of the block: fe_min(ref) < fe_max(query);
// every other block is never met.  The same stored far2_nn decides "not ring 1" and "ring 1", so whatever the bounds are --
// +inf, 0, equal, far2_hd below far2_nn -- a block is in exactly one of the four classes.
enum WideNnRing { kWideRingSeed = 0, kWideRing1 = 1, kWideRing2 = 2, kWideRingNever = 3 };

DC_PRUNE_FN bool wide_nn_is_seed(unsigned query_block, unsigned ref_block) {
  return (ref_block >= query_block ? ref_block - query_block : query_block - ref_block) <= 1u;
}

// The cross form has two orders, so "the blocks next to the query block" do not exist: the seed of a query
// block is ONE reference block, the one with a live row whose box centre is nearest to the query block's box centre in
// the plane, the lowest block on a tie.  The key of a reference block: (bits of c2) << 32 | block, c2 = the two
// differences of the centres 0.5f * (lo + hi), their squares, one sum; the seed is the block of the least key.  c2 >= +0
// or a NaN, so its bits order as the numbers do; a block without a live row (lo > hi) gets the high word ~0 and loses to
// every block with one.  Whatever the data, the least key names a block that was scanned.
DC_PRUNE_FN unsigned long long wide_cross_seed_key(const WideBox& query, const WideBox& ref, unsigned ref_block) {
  unsigned bits = 0xFFFFFFFFu;
  if (!(ref.lo0 > ref.hi0) && !(ref.lo1 > ref.hi1)) {
    const float dx = 0.5f * (query.lo0 + query.hi0) - 0.5f * (ref.lo0 + ref.hi0);
    const float dy = 0.5f * (query.lo1 + query.hi1) - 0.5f * (ref.lo1 + ref.hi1);
    const float c2 = dx * dx + dy * dy;
    __builtin_memcpy(&bits, &c2, sizeof(bits));
  }
  return ((unsigned long long)bits << 32) | ref_block;
}
DC_PRUNE_FN bool wide_cross_is_seed(unsigned seed_of_query_block, unsigned ref_block) { return ref_block == seed_of_query_block; }

// B: the largest exact d2 among the block's live rows so far (+inf: a row has none).  1.0001 as wide_prune_far2; below
// the smallest normal float the relative bounds of the proof do not hold, so the bound never falls below it (B = 0, a
// block of duplicates, keeps the blocks at gap 0: a duplicate of a lower row may sit in any of them).  floor:
// wide_nn_floor of the width; the default is the rule of 65..256 columns
DC_PRUNE_FN float wide_nn_far2(float B, float floor = 1.17549435e-38f) { return 1.0001f * fmaxf(B, floor); }

DC_PRUNE_FN int wide_nn_ring(bool seed, float gap2, float far2_nn, float far2_hd, float fe_min_ref, float fe_max_query) {
  if (seed) return kWideRingSeed;
  if (gap2 < far2_nn) return kWideRing1;
  if (gap2 < far2_hd && fe_min_ref < fe_max_query) return kWideRing2;
  return kWideRingNever;
}
