// dc_reference_layout.hpp -- where the resident reference of the pruned cross sweeps (dc_hip_reference_*, rows of 1..64
// columns) keeps its arrays.  Host arithmetic only, behind dc_mfma_kernels.hpp (nm_for, align256,
// kHdrBytes) inside namespace dc::{anonymous}: dc_mfma.hip lays its workspace out by it, and
// scratch/reference_layout_check.hip walks it over a few thousand shapes under the host sanitizers.
//
// Three regions behind the header and the resident words:
//   resident (n_ref, n_cols)    the reference twice, once per sweep -- the two sweeps order it by different cells and read
//                               different images at different scales:
//                                 populations  cell order at kPopCellFrames: the order, the gathered rows, a box per tile,
//                                              the plain A image and the norms at the population scale
//                                 neighbours   (cell, quantised free energy) order at kNnCellFrames: the order, the
//                                              gathered rows, a box per tile, the FOLDED A image at the neighbour scale,
//                                              the free energies by position, their range per tile, against_meta_kernel's
//                                              words, the free energies by row (the direct kernel's), and the +inf
//                                              words a sweep without free energies reads (as a per-call sweep forms them)
//   batch (max_batch, n_cols)   per sweep the batch's order, a box per tile, the B image and the norms at that sweep's
//                               scale; the merge words of the neighbour sweep's shares; the neighbour grid's keys and
//                               values, which the gate writes and the second sort of a stage consumes
//   scratch (the larger count)  keys, sorted keys, values and the sort's own bytes: the reference's sorts, then a batch's.
// Nothing that outlives a sort lies in the scratch, nothing a sweep writes lies in the resident region, and the two sweeps
// write nothing the other reads (the header's counters and scale words apart, which the arm kernel sets in front of each).
#pragma once

constexpr size_t kRefWordsBytes = 512;                       // the resident words, behind the header (dc_reference.hpp)
constexpr size_t kRefOffArrays = kHdrBytes + kRefWordsBytes; // where the resident region begins

struct ReferenceSide {   // one sweep's view of the reference and of a batch
  size_t off_img_r, off_norm_r, off_perm_r, off_coords_r, off_box_r;
  size_t off_img_q, off_norm_q, off_perm_q, off_box_q;
};
struct ReferenceLayout {
  uint32_t T_r, T_q, NM;   // tiles of the reference, of a batch of max_batch rows; MFMAs per tile pair
  ReferenceSide pop, nn;
  size_t off_fe_c, off_ferange, off_meta, off_fe_row;   // the neighbour side of the reference
  size_t off_fe_c_none, off_ferange_none;               // ... and what a sweep without free energies reads in their place (+inf)
  size_t off_merge64, off_keys_nn, off_vals_nn;         // the neighbour side of a batch
  size_t off_keys_in, off_keys_out, off_vals_in, off_sort, sort_bytes;
  size_t resident_begin, resident_end, batch_begin, batch_end, total;   // scratch: batch_end .. total
};

inline ReferenceLayout reference_layout(size_t n_ref, size_t n_cols, size_t max_batch) {
  ReferenceLayout R{};
  R.T_r = (uint32_t)((n_ref + 31) / 32);
  R.T_q = (uint32_t)((max_batch + 31) / 32);
  R.NM = (uint32_t)nm_for((int)n_cols);
  const size_t tile_bytes = (size_t)16 * 64 * R.NM;
  const size_t pos_r = (size_t)32 * R.T_r, pos_q = (size_t)32 * R.T_q;
  const size_t n_max = max_batch > n_ref ? max_batch : n_ref;
  size_t at = kRefOffArrays;
  auto take = [&at](size_t bytes) {
    const size_t off = at;
    at = align256(at + bytes);
    return off;
  };
  R.resident_begin = at;
  for (ReferenceSide* S : {&R.pop, &R.nn}) {
    S->off_img_r = take(tile_bytes * R.T_r);
    S->off_norm_r = take(sizeof(float) * pos_r);   // (the folded image carries its norms: the neighbour side's stay unused)
    S->off_perm_r = take(sizeof(uint32_t) * pos_r);
    S->off_coords_r = take(sizeof(float) * pos_r * n_cols);
    S->off_box_r = take(sizeof(float) * 4 * (size_t)R.T_r);
  }
  R.off_fe_c = take(sizeof(float) * pos_r);
  R.off_ferange = take(sizeof(float) * 2 * (size_t)R.T_r);
  R.off_meta = take(256);
  R.off_fe_row = take(sizeof(float) * n_ref);
  R.off_fe_c_none = take(sizeof(float) * pos_r);
  R.off_ferange_none = take(sizeof(float) * 2 * (size_t)R.T_r);
  R.resident_end = R.batch_begin = at;
  for (ReferenceSide* S : {&R.pop, &R.nn}) {
    S->off_img_q = take(tile_bytes * R.T_q);
    S->off_norm_q = take(sizeof(float) * pos_q);
    S->off_perm_q = take(sizeof(uint32_t) * pos_q);
    S->off_box_q = take(sizeof(float) * 4 * (size_t)R.T_q);
  }
  R.off_merge64 = take(sizeof(unsigned long long) * 2 * pos_q);
  R.off_keys_nn = take(sizeof(uint32_t) * max_batch);
  R.off_vals_nn = take(sizeof(uint32_t) * max_batch);
  R.batch_end = at;
  R.off_keys_in = take(sizeof(uint32_t) * n_max);
  R.off_keys_out = take(sizeof(uint32_t) * n_max);
  R.off_vals_in = take(sizeof(uint32_t) * n_max);
  R.sort_bytes = sort_temp_bytes(n_max);
  R.off_sort = take(R.sort_bytes);
  R.total = at;
  return R;
}
