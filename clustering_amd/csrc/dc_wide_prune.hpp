// The survivor rule of the pruned wide population sweep: which reference blocks a query block has to meet.
// Every block of 128 positions of the spatial order keeps the box of its rows in the (col 0, col 1) plane, the original
// floats; a reference block survives the scan of a query block iff
//     box_gap2(query box, reference box)  <  far2 = 1.0001f x (the largest fl32(r^2) of the launch),
// the rule of pop_pruned_kernel.  A pair of frames is at least as far apart as the boxes of its blocks, so a block that
// does not survive holds no pair inside any radius of the launch -- with the roundings of the gap and of the canonical
// sum of up to 256 columns inside the margin (the proof: DESIGN §4.22).
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

// r2max: the largest fl32(r^2) of the launch (a number >= 0 or +inf; a NaN radius came in as 0)
DC_PRUNE_FN float wide_prune_far2(float r2max) { return 1.0001f * r2max; }

// r2 = 0 keeps nothing (no pair has d2 < 0), r2 = +inf every block with a live row
DC_PRUNE_FN bool wide_prune_survives(const WideBox& query, const WideBox& ref, float far2) {
  return wide_box_gap2(query, ref) < far2;
}
