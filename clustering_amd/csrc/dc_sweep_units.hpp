// Placement of the per-wave pruned sweeps' units (pop_pruned_kernel, nn_pruned_kernel).  A UNIT is what one
// workgroup does: one block of consecutive query groups (block unit, in spatial order) x one reference share.  The block
// units are cut into eight contiguous EIGHTHS; eighth e of share y belongs to XCD label (e - y) & 7, so that the groups
// running side by side on an XCD stream the same reference tiles through its L2, and every label meets every eighth.
//   static   one workgroup per unit: block (x, y) of a grid of (n_blocks rounded up to 8) x n_chunks runs xcd_unit(x, y)
//   tickets  persistent workgroups draw (queue, ticket) pairs; queue q holds, share after share, exactly the units the
//            blocks with x & 7 == q run in the static form, in the order the dispatcher starts them
// Plain C++ that compiles for the device and for the host (tests/cpp/test_sweep_units.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_UNITS_FN __host__ __device__ __forceinline__
#else
#define DC_UNITS_FN inline
#endif

constexpr uint32_t kNoUnit = 0xFFFFFFFFu;
constexpr uint32_t kSweepQueues = 8;   // one per XCD label (linear workgroup id & 7)

// block units of eighth e, and the first of them
DC_UNITS_FN uint32_t eighth_len(uint32_t n_blocks, uint32_t e) { return (n_blocks >> 3) + (e < (n_blocks & 7u) ? 1u : 0u); }
DC_UNITS_FN uint32_t eighth_first(uint32_t n_blocks, uint32_t e) {
  const uint32_t rem = n_blocks & 7u;
  return e * (n_blocks >> 3) + (e < rem ? e : rem);
}

// static form: the block unit of workgroup (bx, by); kNoUnit for a pad block of the grid
DC_UNITS_FN uint32_t xcd_unit(uint32_t n_blocks, uint32_t bx, uint32_t by) {
  const uint32_t phys = bx & 7u, idx = bx >> 3;
  const uint32_t eighth = (phys + by) & 7u;
  if (idx >= eighth_len(n_blocks, eighth)) return kNoUnit;
  return eighth_first(n_blocks, eighth) + idx;
}

struct SweepUnit {
  uint32_t blk, share;   // blk == kNoUnit: the ticket lies past the end of its queue
};
// units of queue q: the eighths (q + y) & 7 of the shares y = 0 .. n_chunks - 1
DC_UNITS_FN uint32_t sweep_queue_len(uint32_t n_blocks, uint32_t n_chunks, uint32_t q) {
  uint32_t len = (n_chunks >> 3) * n_blocks;   // (eight consecutive shares: every eighth once)
  for (uint32_t y = n_chunks & ~7u; y < n_chunks; ++y) len += eighth_len(n_blocks, (q + y) & 7u);
  return len;
}
// the ticket-th unit of queue q
DC_UNITS_FN SweepUnit sweep_unit(uint32_t n_blocks, uint32_t n_chunks, uint32_t q, uint32_t ticket) {
  SweepUnit u{kNoUnit, 0u};
  if (n_blocks == 0) return u;
  const uint32_t cyc = ticket / n_blocks;
  uint32_t r = ticket - cyc * n_blocks;
  if (cyc >= (n_chunks + 7u) >> 3) return u;   // (also keeps 8 * cyc from wrapping)
  for (uint32_t y = 8u * cyc; y < n_chunks; ++y) {   // (at most eight trips: r < n_blocks = the eight eighths together)
    const uint32_t e = (q + y) & 7u, len = eighth_len(n_blocks, e);
    if (r < len) {
      u.blk = eighth_first(n_blocks, e) + r;
      u.share = y;
      return u;
    }
    r -= len;
  }
  return u;
}
