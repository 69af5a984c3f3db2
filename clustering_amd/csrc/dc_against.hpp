// dc_against.hpp -- the pruned matrix-core population sweep of new frames against a reference
// (DC_VARIANT_CROSS_PRUNED, dc_hip_populations_cross_dev): host-side entry points.  The preparation (one cell grid
// for both sets, the two orders, images, boxes) is dc_mfma.hip / dc_prep.hpp, the sweep kernel dc_against.hip.
#pragma once
#include "dc_mfma.hpp"

namespace dc {

// where the preparation leaves the operands of one pruned cross sweep
struct AgainstArgs {
  const float* qcoords;      // the caller's query rows (gathered by frame for the exact path)
  const uint4* img_r;        // A form of R in cell order, T_r tiles
  const float* norms_r;
  const float4* box_r;       // per tile (lo0, hi0, lo1, hi1); an all-pad tile is empty (infinitely far)
  const float* coords_r;     // R's rows gathered into the order
  const uint4* img_q;        // B form of the rows [i_from, i_to) of Q in cell order, T_q tiles
  const float* norms_q;
  const uint32_t* perm_q;    // position -> query row, kInvalidFrame for the pad positions
  const float4* box_q;
  uint32_t T_r, T_q;
  uint32_t n_q;              // rows of the caller's query array (stride of pops)
  const uint32_t* hdr;
  unsigned long long* chain_counter;   // header words 2..3 (evaluated tile pairs), + kMfmaCtrPop: issued MFMAs
};

// true if the pruned cross sweep takes this call; otherwise the every-pair sweep answers in the same workspace
bool cross_pruned_takes(size_t n_ref, size_t n_cols);
// bytes of the pruned layout (never less than cross_workspace_bytes); 0 if n_cols has no matrix-core sweep
size_t cross_pruned_workspace_bytes(size_t n_q, size_t n_ref, size_t n_cols);
// as launch_pop_cross_mfma, tile pairs farther apart than the call's largest radius skipped
int launch_pop_cross_pruned(const float* d_query, uint32_t n_q, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                            uint32_t i_from, uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops, void* d_ws,
                            hipStream_t stream);
// dc_against.hip: one radius (rad2.v[0]) on a finished preparation; pops [n_q] zero-filled by the caller
void pop_against_sweep(const AgainstArgs& A, uint32_t n_cols, const Rad2& rad2, uint32_t* pops, hipStream_t s);

}  // namespace dc
