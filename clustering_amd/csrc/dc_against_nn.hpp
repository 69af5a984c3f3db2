// dc_against_nn.hpp -- the pruned matrix-core NEIGHBOUR sweep of new frames against a reference
// (dc_hip_nearest_neighbors_cross_pruned_dev): host-side entry points.  The preparation (one cell grid for both sets,
// R ordered by (cell, free energy), images, boxes, free-energy ranges) is dc_mfma.hip / dc_prep.hpp, the sweep kernel
// and the merge of its reference shares dc_against_nn.hip.
#pragma once
#include "dc_mfma.hpp"

namespace dc {

constexpr size_t kNnAgainstInfoBytes = 128;   // the header words dc_hip_nearest_cross_pruned_info_dev reads (0 .. 31)

// where the preparation leaves the operands of one pruned cross neighbour sweep
struct NnAgainstArgs {
  const float* qcoords;      // the caller's query rows (gathered by frame for the exact path)
  const float* fe_q;         // by query row; nullptr: nn only (nn_hd is closed for every query)
  const uint4* img_r;        // folded A form of R in (cell, free energy) order, T_r tiles
  const uint32_t* perm_r;    // position -> reference row, kInvalidFrame for the pad positions
  const float4* box_r;       // per tile (lo0, hi0, lo1, hi1); an all-pad tile is empty (infinitely far)
  const float2* ferange_r;   // per tile [fe_lo, fe_hi] of its real rows
  const float* fe_c;         // free energies gathered into the order, +inf on the pad positions
  const float* coords_r;     // R's rows gathered into the order
  const uint4* img_q;        // B form of the rows [i_from, i_to) of Q in cell order, T_q tiles
  const float* norms_q;
  const uint32_t* perm_q;    // position -> query row, kInvalidFrame for the pad positions
  const float4* box_q;
  const float* meta;         // [0..3]: bounding box of R in the (col 0, col 1) plane, [4]: squared cell edge of the grid
  unsigned long long* merge64;   // [2][32 T_q] by query POSITION: the merge of several reference shares
  uint32_t T_r, T_q, n_ref;
  uint32_t* hdr;             // words 4..5: evaluated tile pairs, 26..27: issued MFMAs, kHdrShares (dc_mfma_kernels.hpp)
};

// bytes of the pruned layout (never less than cross_workspace_bytes); 0 if n_cols has no matrix-core sweep
size_t nn_cross_pruned_workspace_bytes(size_t n_q, size_t n_ref, size_t n_cols);
// as launch_nn_cross_mfma, reference tiles visited in rings of growing box distance from each query group; a reference
// the candidate queue cannot address (cross_pruned_takes) goes to launch_nn_cross_mfma in the same workspace
int launch_nn_cross_pruned(const float* d_query, uint32_t n_q, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                           const float* d_fe_q, const float* d_fe_r, uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx,
                           float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t stream);
// dc_against_nn.hip: the sweep on a finished preparation; outputs by query row (d_hd_* may be nullptr with fe_q)
void nn_against_sweep(const NnAgainstArgs& A, uint32_t n_cols, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx,
                      float* hd_d2, hipStream_t s);

}  // namespace dc
