// dc_mfma_wide.hpp -- the matrix-core sweeps for rows of 65..256 columns (dc_mfma_wide.hip): host-side entry points.
// An every-pair self sweep whose K axis streams through LDS in chunks while the accumulator tiles stay in registers
// (kernels and the reasoning: dc_mfma_wide_kernels.hpp; the radius graph on the same sweep: 4.20).  Entry
// points of their own in the C ABI (dc_hip_*_wide_dev); no variant value selects them.
#pragma once
#include "dc_common.hpp"

namespace dc {

constexpr size_t kWideMinCols = 65, kWideMaxCols = 256;
inline bool wide_mfma_supports(size_t n_cols) { return n_cols >= kWideMinCols && n_cols <= kWideMaxCols; }
// bytes of device scratch (header, column means, both operand images, norms, the neighbour merge words); 0 if the
// column count is not served or there are no rows; monotone in n_rows
size_t wide_workspace_bytes(size_t n_rows, size_t n_cols);
constexpr size_t kWideInfoBytes = 256;   // the head of the workspace dc_hip_wide_info_dev reads (header words 40..45)

// ---- rows of 257..1024 columns (dc_hip_*_xwide_dev) --------------------------------------------------------
// The unpruned self and cross sweeps below serve these widths as they stand: the chain streams along K and takes its
// length at run time.  What differs is the workspace -- the sums and means regions behind the header hold kXWideMaxCols
// entries, so the images start further back -- and with it the byte counts; wide_prepare, launch_*_wide_mfma,
// wide_prepare_against and launch_*_wide_against read the layout of the width they are given.
constexpr size_t kXWideMinCols = kWideMaxCols + 1, kXWideMaxCols = 1024;
inline bool xwide_mfma_supports(size_t n_cols) { return n_cols >= kXWideMinCols && n_cols <= kXWideMaxCols; }
// as wide_workspace_bytes / wide_against_workspace_bytes: 0 if the column count is not served or a set is empty
size_t xwide_workspace_bytes(size_t n_rows, size_t n_cols);
size_t xwide_against_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols);

// statistics, scale and operand images of d_coords in the workspace (d_fe: the neighbour call's free energies, a NaN
// among them flags the data like a non-finite row); returns 0 on success
int wide_prepare(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, void* d_ws,
                 hipStream_t stream);
// populations of the rows [i_from, i_to) for up to kMaxRadiiPerLaunch radii with ONE chain per tile pair, ADDED to
// d_pops_first_row (zeroed by the caller); stands down on flagged data (the gated direct kernel answers)
void launch_pop_wide_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                          const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row, void* d_ws, hipStream_t stream);
// nn / nn_hd of the rows [i_from, i_to) (outputs preset to "none" by the caller); stands down on flagged data
int launch_nn_wide_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, uint32_t i_from,
                        uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2,
                        void* d_ws, hipStream_t stream);

// ---- the radius graph at one threshold r2 = the squared distance itself (dc_hip_radius_*_wide_dev) ------
// Both run behind wide_prepare in the same workspace, ADD the populations to d_pops (zeroed by the caller) and stand down
// on flagged data (the gated launch_pairs_direct / launch_min_edge_direct answer).
// every unordered pair once into d_pairs[0 .. capacity) (nullptr: counting only), the number found ADDED to d_count
void launch_pairs_wide_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2, uint32_t* d_pops, uint2* d_pairs,
                            unsigned long long capacity, unsigned long long* d_count, void* d_ws, hipStream_t stream);
// what the queries [i_from, i_to) see of one Boruvka round: atomicMin into d_best (preset to ~0 by the caller)
void launch_min_edge_wide_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2, const uint32_t* d_comp,
                               const uint32_t* d_rank, uint32_t i_from, uint32_t i_to, unsigned long long* d_best,
                               uint32_t* d_pops, void* d_ws, hipStream_t stream);

// ---- the pruned self population sweep (dc_hip_populations_wide_pruned_dev) --------------------------------
// The rows in a spatial order on columns 0 / 1 (cell keys, one stable sort), gathered once into that order, a box per
// block of 128 positions; a workgroup scans the boxes of its share and runs the chains of the blocks that can hold a
// pair within the launch's largest radius (dc_wide_prune.hpp).  Counts by position, scattered to the rows behind the sweep.
// bytes: the workspace of the unpruned sweeps at its head (header, images, norms), then the order, the gathered rows, the
// boxes, the counts and the sort's scratch; 0 if the column count is not served or there are no rows; monotone in n_rows
size_t wide_pruned_workspace_bytes(size_t n_rows, size_t n_cols);
// ... and of the pruned self population and neighbour sweeps at 257..1024 columns (dc_hip_*_xwide_pruned_dev, DESIGN.md
// 4.33): the same regions behind the head of those widths; 0 outside them.  wide_pruned_prepare, launch_pop_wide_pruned,
// launch_nn_wide_pruned and wide_pruned_order serve both families and read the layout of the width they are given; the
// pruning rules take the floors of the width (dc_wide_prune.hpp)
size_t xwide_pruned_workspace_bytes(size_t n_rows, size_t n_cols);
// statistics, order, gathered rows, boxes and images, on the stream, no host synchronisation; returns 0 on success
// (d_fe: the neighbour call's free energies, a NaN among them flags the data like a non-finite row)
int wide_pruned_prepare(const float* d_coords, uint32_t n_rows, uint32_t n_cols, void* d_ws, hipStream_t stream,
                        const float* d_fe = nullptr);
// the populations of the query blocks segment, segment + n_segments, ... of the order (n_segments >= 1) for up to
// kMaxRadiiPerLaunch radii, WRITTEN to d_pops_first_row for every row (zeros for the rows of other blocks); stands down
// on flagged data, scatter included (the gated direct kernel answers).  Returns 0 on success.
int launch_pop_wide_pruned(uint32_t n_rows, uint32_t n_cols, size_t segment, size_t n_segments, const Rad2& rad2, int n_rad,
                           uint32_t* d_pops_first_row, void* d_ws, hipStream_t stream);
// the order the workspace holds, position -> row, copied to d_perm; 0 ok, 1 the workspace holds no order of that shape,
// -1 a HIP error (synchronises)
int wide_pruned_order(const void* d_ws, uint32_t n_rows, uint32_t n_cols, uint32_t* d_perm, hipStream_t stream);

// ---- the pruned radius graph (dc_hip_radius_*_wide_pruned_dev) --------------------------------------------
// The pruned sweep of ONE threshold r2 = the squared distance itself, with the sinks of the radius graph.  Both run behind
// wide_pruned_prepare in the same workspace (wide_pruned_workspace_bytes: rows 1 and 2 of its count region hold comp and
// rank gathered into the order), WRITE the populations to d_pops for every row and stand down on flagged data, scatter
// included (the gated launch_pairs_direct / launch_min_edge_direct answer).  Return 0 on success.
// every unordered pair once into d_pairs[0 .. capacity) as rows, in no order -- neither of the list nor within a pair --
// (nullptr: counting only), the number found ADDED to d_count
int launch_pairs_wide_pruned(uint32_t n_rows, uint32_t n_cols, float r2, uint32_t* d_pops, uint2* d_pairs,
                             unsigned long long capacity, unsigned long long* d_count, void* d_ws, hipStream_t stream);
// what the queries of the blocks segment, segment + n_segments, ... of the order (n_segments >= 1) see of one Boruvka
// round: atomicMin into d_best (preset to ~0 by the caller); d_comp / d_rank are by row, as the caller holds them
int launch_min_edge_wide_pruned(uint32_t n_rows, uint32_t n_cols, float r2, const uint32_t* d_comp, const uint32_t* d_rank,
                                size_t segment, size_t n_segments, unsigned long long* d_best, uint32_t* d_pops, void* d_ws,
                                hipStream_t stream);
// ---- the pruned self neighbour sweep (dc_hip_nearest_neighbors_wide_pruned_dev) ---------------------------
// Behind wide_pruned_prepare(.., d_fe) in the same workspace: nn / nn_hd of the query blocks segment, segment + n_segments,
// ... of the order (n_segments >= 1), WRITTEN to the rows of those blocks (outputs preset to "none" by the caller, where
// the rows of other blocks stay); three pruned launches -- seed blocks, ring 1, ring 2 (dc_wide_prune.hpp) -- whose
// counters add up; stands down on flagged data, finish included (the gated direct kernel answers).  Returns 0 on success.
int launch_nn_wide_pruned(const float* d_fe, uint32_t n_rows, uint32_t n_cols, size_t segment, size_t n_segments,
                          uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws,
                          hipStream_t stream);
// the three counters of the last sweep back to zero (a further round in a workspace that stays prepared)
int wide_clear_counters(void* d_ws, hipStream_t stream);

// ---- neighbour blocks of a sharded run in the order of that sweep (dc_hip_neighbors_block_*_wide_dev) -----
// Behind a segment call of launch_nn_wide_pruned in the same workspace: the rows of the query blocks segment, segment +
// n_segments, ... compacted by local position into [4][wide_nn_block_rows] (nn_idx, nn_d2 bits, hd_idx, hd_d2 bits; pads hold
// "none"), the last 32 entries of plane 0 being the layout header; on flagged data the reference's row block instead,
// decided on the device from the word the sweep's gate read.  No host synchronisation; return 0 on success.
// rows of a block: the larger of the largest segment in positions and the largest row block, plus the header; 0 if the
// column count is not served, for no rows and for no segments
size_t wide_nn_block_rows(size_t n_rows, size_t n_cols, size_t n_segments);
// ... of 257..1024 columns (dc_hip_neighbors_block_*_xwide_dev): the same number, 0 outside those widths.
// The pack, the unpack and the status below serve both families, in the layout of the width they are given
size_t xwide_nn_block_rows(size_t n_rows, size_t n_cols, size_t n_segments);
int launch_nn_block_pack_wide(const uint32_t* d_nn_idx, const float* d_nn_d2, const uint32_t* d_hd_idx, const float* d_hd_d2,
                              uint32_t n_rows, uint32_t n_cols, uint32_t segment, uint32_t n_segments, void* d_ws, uint32_t* d_block,
                              hipStream_t stream);
// [n_segments][4][wide_nn_block_rows] -> the four arrays by row.  The kernel compares the headers of all blocks with the
// layout of this workspace first; on a mismatch it writes nothing and leaves the verdict in the header (wide_layout_status)
int launch_nn_block_unpack_wide(const uint32_t* d_blocks, uint32_t n_rows, uint32_t n_cols, uint32_t n_segments, void* d_ws,
                                uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, hipStream_t stream);
// the verdict of the last unpack in the workspace (1: refused); synchronises; 0 ok, -1 a HIP error
int wide_layout_status(const void* d_ws, int* mismatch, hipStream_t stream);

// ---- the cross form: query rows against a reference (dc_hip_*_cross_wide_dev) -----------------------------
// The same kernel in its kAgainst instances: one origin and one scale over both sets, the A form and the norms of the
// reference, the B form and the merge words of the queries; every pair counts (no self term, no exclusion).
// bytes of device scratch; 0 if the column count is not served or either set is empty; monotone in either row count
size_t wide_against_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols);
int wide_prepare_against(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                         void* d_ws, hipStream_t stream);
// ADDED to d_pops_first_row ([n_rad][n_query], zeroed by the caller); stands down on flagged data
void launch_pop_wide_against(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                             uint32_t i_from, uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row,
                             void* d_ws, hipStream_t stream);
// outputs preset to "none" by the caller; d_fe_query == nullptr: nn only (d_fe_ref and the hd outputs are not touched)
int launch_nn_wide_against(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                           const float* d_fe_query, const float* d_fe_ref, uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx,
                           float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t stream);

// ---- the pruned cross population sweep (dc_hip_populations_cross_wide_pruned_dev) -------------------------
// The statistics of the cross form (one origin, one scale over both arrays), then ONE cell grid on columns 0 / 1 over the
// query range and the reference together, its cell sized by the reference's row count; the reference and the query range
// each sorted by those keys, gathered, boxed per block of 128 positions and imaged (A form and norms: reference, B form:
// queries).  A workgroup owns (block of the query order, reference share), scans the reference's boxes against its query
// box and runs the chains of the survivors; counts by query position, scattered to the rows behind the sweep.
// bytes: the workspace of the unpruned cross sweeps at its head, then both orders, the sort's keys, both gathered sets, both
// sets of boxes, the counts and the sort's scratch; 0 if the column count is not served or either set is empty; monotone
// in either row count
size_t wide_cross_pruned_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols);
// ... and of the pruned cross population and neighbour sweeps at 257..1024 columns (dc_hip_*_cross_xwide_pruned_dev,
// DESIGN.md 4.34): the same regions behind the head of those widths; 0 outside them.  wide_cross_pruned_prepare,
// launch_pop_wide_cross_pruned, launch_nn_wide_cross_pruned and wide_cross_pruned_order serve both families and read the
// layout of the width they are given; the pruning rules take the floors of the width (dc_wide_prune.hpp)
size_t xwide_cross_pruned_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols);
// on the stream, no host synchronisation; i_from < i_to <= n_query, n_ref > 0; returns 0 on success
int wide_cross_pruned_prepare(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                              uint32_t i_from, uint32_t i_to, void* d_ws, hipStream_t stream);
// the populations of the queries [i_from, i_to) -- the range the workspace was prepared for -- for up to kMaxRadiiPerLaunch
// radii, WRITTEN to those rows of d_pops_first_row ([n_rad][n_query]; the other rows are the caller's); stands down on
// flagged data, scatter included (the gated direct kernel answers).  Returns 0 on success.
int launch_pop_wide_cross_pruned(uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                                 const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row, void* d_ws, hipStream_t stream);
// ---- the pruned cross neighbour sweep (dc_hip_nearest_neighbors_cross_wide_pruned_dev) --------------------
// Behind wide_cross_pruned_prepare(.., i_from, i_to, ..) in the same workspace: nn / nn_hd of the queries [i_from, i_to)
// against the reference, WRITTEN to those rows (outputs preset to "none" by the caller).  Three launches of the pruned
// kAgainst neighbour instance -- the seed block of every query block (the reference block whose box centre is nearest,
// dc_wide_prune.hpp), ring 1, ring 2 -- whose counters add up; d_fe_query == nullptr: nn only, two launches, the hd outputs
// are not touched.  A NaN free energy flags the data (the gathers of the free energies raise the flag); on flagged data the
// launches and the finish stand down (the gated direct kernel answers).  Uses the sort's key arrays of the layout, so its byte count is wide_cross_pruned_workspace_bytes.  Returns 0 on success.
int launch_nn_wide_cross_pruned(uint32_t n_query, uint32_t n_ref, uint32_t n_cols, const float* d_fe_query, const float* d_fe_ref,
                                uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                float* d_hd_d2, void* d_ws, hipStream_t stream);
// both orders the workspace holds, position -> row, copied to d_perm_q ([n_query_range], rows of the query array) and
// d_perm_r ([n_ref]); 0 ok, 1 the workspace holds no cross order of that shape, -1 a HIP error (synchronises)
int wide_cross_pruned_order(const void* d_ws, uint32_t n_query_range, uint32_t n_ref, uint32_t n_cols, uint32_t* d_perm_q,
                            uint32_t* d_perm_r, hipStream_t stream);

// ---- the resident reference of the pruned cross sweeps (dc_hip_reference_wide_*) --------------------------
// The reference prepared once under statistics of its own (origin: its column means; scale: that of four times its
// largest |x - mean|^2; grid: its extent), a batch of at most max_batch queries staged against it in one pass (the gate:
// a row that is non-finite or beyond the scale's extent flags the batch, which the gated direct kernels then answer),
// and the two pruned cross sweeps in that workspace, in any order and any number of times per staged batch.  Everything
// runs on the stream without host synchronisation, except the two readers.  All return 0 on success.
// bytes: a resident region sized by (n_ref, n_cols), a batch region sized by (max_batch, n_cols), the sort's scratch sized
// by the larger count; 0 if the column count is not served or a count is zero; monotone in each argument
size_t wide_reference_workspace_bytes(size_t n_ref, size_t n_cols, size_t max_batch);
// ... of the third kind, rows of 257..1024 columns (dc_hip_reference_xwide_*): 0 outside those widths.  The
// functions below read the layout of the width they are given and serve both kinds
size_t xwide_reference_workspace_bytes(size_t n_ref, size_t n_cols, size_t max_batch);
int wide_reference_open(const float* d_ref, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, void* d_ws, hipStream_t stream);
// the reference's free energies: copied by row (what the direct kernel reads), gathered by position, the least per block;
// a NaN among them raises a word of its own, which only a neighbour sweep with free energies reads
int wide_reference_set_free_energies(const float* d_fe_ref, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, void* d_ws,
                                     hipStream_t stream);
const float* wide_reference_fe_by_row(const void* d_ws, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch);
// the batch half: gate and keys, order, gathered rows, boxes, B image (n_query <= max_batch; 0: only the batch's words are cleared)
int wide_reference_stage(const float* d_query, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, void* d_ws,
                         hipStream_t stream);
// in front of a population sweep: header word 1 from the reference's and the batch's flags, the counters from zero
// (launch_nn_wide_reference does the same itself, with the free energies' flags)
int wide_reference_arm(void* d_ws, hipStream_t stream);
// launch_pop_wide_cross_pruned / launch_nn_wide_cross_pruned of the staged batch (d_fe_query == nullptr: nn only)
int launch_pop_wide_reference(uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, const Rad2& rad2, int n_rad,
                              uint32_t* d_pops_first_row, void* d_ws, hipStream_t stream);
int launch_nn_wide_reference(uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, const float* d_fe_query,
                             uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t stream);
// the counters of the last sweep and who answered it; both orders, position -> row (a null pointer is skipped); synchronise
int wide_reference_info(const void* d_ws, uint64_t* tiles, uint64_t* mfmas, uint64_t* exact_pairs, uint32_t* answered,
                        hipStream_t stream);
int wide_reference_order_copy(const void* d_ws, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch,
                              uint32_t* d_perm_q, uint32_t* d_perm_r, hipStream_t stream);

}  // namespace dc
