// dc_against_ref.hpp -- the resident reference of the pruned cross sweeps for rows of 1..64 columns (dc_hip_reference_*,
// DESIGN.md 4.29): host-side entry points.  The reference's half of the preparation of launch_pop_cross_pruned and
// launch_nn_cross_pruned runs once, under statistics that do not depend on a batch (dc_reference.hpp); a batch's half
// runs per stage; the sweeps are pop_against_sweep and nn_against_sweep as they stand.  Preparation and layout:
// dc_mfma.hip, dc_reference.hpp, dc_reference_layout.hpp.
#pragma once
#include "dc_mfma.hpp"

namespace dc {

// true if a handle can serve this reference: a matrix-core column count and an order the band-pair queue can address
// (cross_pruned_takes; the per-call entry points send a longer reference to the every-pair sweep)
bool reference_takes(size_t n_ref, size_t n_cols);
// bytes of the three regions; 0 if n_cols has no matrix-core sweep or a count is zero
size_t reference_workspace_bytes(size_t n_ref, size_t n_cols, size_t max_batch);
// the reference's statistics, both scales (the population scale for r2max, the largest squared radius of any population
// call), both orders of R with their rows, boxes and images; the neighbour side in its cell-only form.  0 on success.
int reference_open(const float* d_ref, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, float r2max, void* d_ws,
                   hipStream_t s);
// a copy of fe_ref by row, and the neighbour side of R again in (cell, free energy) order
int reference_set_free_energies(const float* d_ref, const float* d_fe_ref, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch,
                                void* d_ws, hipStream_t s);
const float* reference_fe_by_row(const void* d_ws, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch);
// a batch: the gate, and both of its orders with their boxes and B images
int reference_stage(const float* d_query, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, void* d_ws,
                    hipStream_t s);
// the population sweep of the staged batch, one launch per squared radius; d_pops [n_rad][n_query] zero-filled by the caller
int launch_pop_reference(const float* d_query, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch,
                         const float* rad2, int n_rad, uint32_t* d_pops, void* d_ws, hipStream_t s);
// the neighbour sweep of the staged batch; outputs by query row, initialised by the caller (launch_nn_init)
int launch_nn_reference(const float* d_query, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch,
                        const float* d_fe_query, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2,
                        void* d_ws, hipStream_t s);
// counters of the last sweep and who answered it (synchronises)
int reference_info(const void* d_ws, uint64_t* tiles, uint64_t* mfmas, uint32_t* shares, uint32_t* answered, hipStream_t s);
// the orders of one sweep (which: 0 the population sweep's, 1 the neighbour sweep's), position -> row (synchronises)
int reference_order_copy(const void* d_ws, int which, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch,
                         uint32_t* d_perm_q, uint32_t* d_perm_r, hipStream_t s);

}  // namespace dc
