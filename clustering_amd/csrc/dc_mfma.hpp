// dc_mfma.hpp -- matrix-core variants (fp16x2 Gram form on the f16 MFMA as a classifier + guard band +
// canonical fp32 re-check of the undecided pairs): host-side entry points.
#pragma once
#include "dc_common.hpp"

namespace dc {

// Optional second product of the pruned population sweep: the list of all unordered frame pairs
// within the radius (the radius graph that the reference's screening walks frame by frame,
// density_clustering.cpp:292-332).  Pairs are emitted as positions in the sweep's spatial order,
// (query position, reference position) with reference < query, i.e. every pair exactly once.
struct EdgeSink {
  uint2* edges;                    // nullptr: counting only
  unsigned long long* count;       // total number of pairs found (may exceed capacity)
  unsigned long long capacity;
  // "lightest outgoing pair" variant (one round of a Boruvka minimum spanning forest of the radius
  // graph): comp / rank per position of the sweep's order, best per component id (a position):
  // min over pairs {a in the component, b outside, d2 < r2} of (max(rank_a, rank_b) << 32 | min(..))
  const uint32_t* comp;
  const uint32_t* rank;
  unsigned long long* best;
};
enum SinkMode { kSinkNone = 0, kSinkPairs = 1, kSinkMinEdge = 2 };

// Measurement and test switches of the matrix-core sweeps, read from the environment once (sweep_switches(),
// dc_mfma.hip); the defaults are the library's behaviour.  The forcing switches move the size thresholds of the planners
// (plan_pop / plan_nn, dc_mfma_kernels.hpp) only within the forms each MFMA count is built for.
struct SweepSwitches {
  bool pop_sym = true;            // DC_POP_SYM=0: no symmetric population sweeps
  int pop_shared = -1;            // DC_POP_SHARED=0 / 1: shared-operand population sweeps off / on where built
  int nn_shared = -1;             // DC_NN_SHARED=0 / 1: the same for the neighbour sweep
  int waves_per_group = 0;        // DC_WAVES_PER_GROUP=1 / 2 / 4: waves per workgroup of the per-wave sweeps
  int nn_coop = -1;               // DC_NN_COOP=0 / 1: COOP neighbour workgroups never / from four shares on
  bool nn_rho = true;             // DC_NN_RHO=0: the neighbour sweep's rings without the radial gap (dc_rho_gap.hpp)
  uint32_t wave_target = 0;       // DC_WAVE_TARGET: waves a pruned launch aims at (0: the sweep's own)
  uint32_t share_floor = 0;       // DC_SHARE_FLOOR: least reference tiles per share (0: the sweep's own)
  bool components = true;         // DC_POP_COMPONENTS=0: one component whatever the data
  float pop_cell_frames = 0.0f;   // DC_POP_CELL_FRAMES / DC_NN_CELL_FRAMES: frames per cell of the orderings (0: default)
  float nn_cell_frames = 0.0f;
  int nn_fe_bits = -1;            // DC_NN_FE_BITS: free-energy bits of the neighbour ordering's key (-1: default)
  uint32_t mfma32_wpb = 1;        // DC_MFMA32_WPB=1 / 2 / 4: waves per workgroup of the fp32-MFMA instance
  uint32_t mfma32_chunks = 0;     // DC_MFMA32_CHUNKS: its reference shares (0: chosen by size)
  bool mfma32_poison_pads = false;   // DC_MFMA32_POISON_PADS=1 (tests): NaN instead of 0 in the pad floats of the fp32 image
  bool tickets = true;            // DC_SWEEP_DISPATCH=static / tickets: the per-wave pruned sweeps on one workgroup per unit /
                                  // on persistent workgroups that draw their units (dc_mfma_kernels.hpp for_each_unit)
  uint32_t sweep_slots = 0;       // DC_SWEEP_SLOTS: most persistent workgroups of a ticketed launch (0: all that can be resident)
};
const SweepSwitches& sweep_switches();
// workgroups of `kernel` (a __global__ function) that can be resident on the current device at once with this block size
// and dynamic LDS: the occupancy query per CU times the CUs, asked once per (device, kernel, block, LDS) and kept
uint32_t sweep_resident_slots(const void* kernel, uint32_t block_threads, size_t dyn_lds);

// The plan of one pruned sweep: which kernel form runs and how its query groups are cut.  The padded orders are laid
// out for group_tiles; the kernel that runs must have the same groups, so both come from the plan.
enum PopForm {
  kPopWave,        // per-wave one-sided (pop_pruned_kernel)
  kPopWaveSym,     // per-wave symmetric: every unordered pair once, counts by position
  kPopPairs,       // per-wave, listing the pairs
  kPopMinEdge,     // per-wave, lightest pair out of every component
  kPopShared,      // reference operands shared through LDS, one-sided (pop_shared_kernel)
  kPopSharedSym,   // ... symmetric
  kPopMsym,        // several radii per sweep, symmetric (pop_msym_kernel)
  kPopMulti,       // several radii per sweep, one-sided (pop_shared_kernel, row ranges)
};
enum NnForm {
  kNnWave,     // per-wave (nn_pruned_kernel); COOP workgroups from coop_shares reference shares per group on
  kNnShared,   // reference operands shared through LDS (nn_shared_kernel)
};
enum CallKind { kCallAll, kCallRange, kCallSegment };   // queries: all rows / a row range / one segment of a sharded run
// operands of one unpruned matrix-core sweep (dc_mfma_kernels.hpp pop_mfma_kernel / nn_mfma_kernel): the query rows
// of Q against every row of R.  A self sweep passes the same frames on both sides (T_q == T_r).
struct SweepArgs {
  const float* qcoords;     // [n_q][n_cols]
  const float* rcoords;     // [n_ref][n_cols]
  uint32_t n_q, n_ref, T_q, T_r;
  const uint4* img_r;       // A form of R: natural order (populations) or ordered by free energy (neighbours)
  const float* norms_r;
  const uint4* img_q;       // B form of Q, natural order
  const float* norms_q;
  const uint32_t* perm;     // neighbours: sorted position -> reference frame
  const uint32_t* invpos;   // self neighbour sweeps: frame -> sorted position
  const uint32_t* pq;       // neighbours: per query, references with strictly lower free energy (nullptr: nn only)
  const uint32_t* hdr;
};

struct PopPlan {
  PopForm form;
  int nr;                  // radii per sweep: 1, 4 or 8
  uint32_t tq;             // query tiles per wave (the kernel's TQ)
  uint32_t group_tiles;    // query tiles per group (the unit of the padded orders and of the segments' deal)
  uint32_t waves;          // waves per workgroup
  int shift_steps;         // thresholds taken off the accumulator in place: the band of the scale pays for them
  bool pos_clean;          // the preparation clears the counts by position (kPopWaveSym)
};
struct NnPlan {
  NnForm form;
  uint32_t tq, group_tiles, waves;
  uint32_t coop_shares;    // kNnWave: reference shares per group from which the shares are the waves of one workgroup
};

// true if the MFMA kernels handle this n_cols
bool mfma_supports(size_t n_cols);
// bytes of device scratch (operand images, norms) for a problem size; 0 if unsupported
size_t mfma_workspace_bytes(size_t n_rows, size_t n_cols);
// builds the operand images of d_coords in the workspace; returns 0 on success
// pruned: a pruned sweep follows (one statistics pass; the component region of the workspace is zero-filled with the
// header unless stats_valid, in which case the statistics of an earlier sweep stay and the sweep clears the region itself)
int mfma_prepare(const float* d_coords, uint32_t n_rows, uint32_t n_cols, void* d_ws, hipStream_t stream,
                 bool stats_valid = false, bool pruned = false, const float* d_fe = nullptr);
// (d_fe: the free energies of a pruned NEIGHBOUR call that claims DC_FLAG_STATS_VALID -- their range and the component
//  guard of that sweep are part of the claim's two launches; launch_nn_pruned[_segment](reuse_components) relies on it)
void launch_pop_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from,
                     uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row,
                     void* d_ws, hipStream_t stream);
// DC_VARIANT_MFMA32 (dc_mfma32.hpp): the fp32-input MFMA instance, n_cols 9..10, every pair (needs mfma_prepare first)
bool mfma32_supports(size_t n_cols);
void launch_pop_mfma32(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                       const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row, void* d_ws, hipStream_t stream);
void launch_nn_mfma32(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, uint32_t i_from,
                      uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws,
                      hipStream_t stream);
// ... and its two orders alone, left in the workspace: the frames by the cells of columns 0 / 1 (L.off_perm), the
// frames by free energy (off_perm, off_invpos, off_pq, off_fe_s); non-zero when the sort failed
int mfma32_order_pop(const float* d_coords, uint32_t n_rows, uint32_t n_cols, void* d_ws, hipStream_t stream);
int mfma32_order_nn(uint32_t n_rows, uint32_t n_cols, const float* d_fe, void* d_ws, hipStream_t stream);

// ---- the same sweeps for n_cols 1..32 and up to 8 radii per pass of the MFMAs (dc_mfma32_general.hip; the entry
// points dc_hip_*_fp32_dev; the workspace of mfma_workspace_bytes; need mfma_prepare first) ------------------------
constexpr size_t kFp32MaxCols = 32;
// How one call is run: decided on the host from the sizes alone (and the DC_MFMA32_* switches), no device involved.
struct Fp32Plan {
  uint32_t steps;            // K-steps of the kernel instance: ceil(n_cols / 2), or one zero step more (fp32_steps)
  uint32_t lane_floats;      // floats per lane and tile of the operand image: steps rounded up to a multiple of four
  uint32_t tq_pop, tq_nn;    // query tiles per wave of the population sweeps of this call and of the neighbour sweep
  uint32_t radii_per_sweep;  // radii that share one pass of the MFMAs
  uint32_t sweeps;           // population sweeps of the call: ceil(n_radii / radii_per_sweep)
  uint32_t chunks_pop, chunks_nn;   // reference chunks (chunks32)
  uint32_t lds_pop, lds_nn;  // dynamic LDS per workgroup, bytes
  uint32_t image_bytes;      // operand image, bytes per tile of 32 rows
  uint32_t region_bytes;     // ... and what make_layout keeps for it
};
bool fp32_supports(size_t n_cols);
uint32_t fp32_steps(size_t n_cols);
// (asserts that image and norms fit the regions of make_layout; n_rows >= 1, n_cols 1..32, n_radii >= 1)
Fp32Plan fp32_plan(size_t n_rows, size_t n_cols, size_t n_radii);
// rad2: the n_radii squared radii of the call in the caller's order (numbers: see radius2 in dc_capi.hip); ONE image,
// scaled for the largest, serves every sweep of the call; d_pops: [n_radii][n_rows], rows [i_from, i_to) written
void launch_pop_fp32(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                     const float* rad2, size_t n_radii, uint32_t* d_pops, void* d_ws, hipStream_t stream);
void launch_nn_fp32(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, uint32_t i_from,
                    uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws,
                    hipStream_t stream);
// population sweep over spatially ordered frames with tile-pair pruning (needs mfma_prepare first)
// comp_clean: mfma_prepare(pruned) of this call has zero-filled the component region of the workspace
void launch_pop_pruned(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from,
                       uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row,
                       void* d_ws, hipStream_t stream, bool comp_clean = false);
// pruned population sweep at squared radius r2 that also lists every unordered frame pair with
// canonical d2 < r2 (frame ids; d_pairs may be nullptr to count only); needs mfma_prepare first.
// *d_count: number of pairs found (> capacity: buffer too small); 0, and nothing written, if the data was flagged
// (the gated launch_pairs_direct answers then).
void launch_radius_pairs(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2,
                         uint32_t* d_pops, uint2* d_pairs, unsigned long long capacity,
                         unsigned long long* d_count, void* d_ws, hipStream_t stream);
// one segment of a sharded sweep: the query groups (TQ consecutive tiles of the sweep's order) are dealt out to the
// segments in BLOCKS of `block` consecutive groups, block-cyclically: segment `offset` of `stride` owns the groups g
// with (g / block) % stride == offset ({1, 0, 1}: all of them).  Dealing cyclically gives every segment the same mix of
// dense and sparse regions (contiguous eighths of C3 differed by up to 16 % in work); dealing whole blocks keeps the
// groups that run side by side on an XCD next to each other in the order, so that they stream the same reference tiles
// through its L2 (group by group -- block 1 -- an eighth of C3 read 3 x the bytes of the unsharded sweep per tile pair
// at the L2's memory side, L2 hit rate 0.76 against 0.91, and its kernels took 12 - 17 % more than an eighth).
struct QSeg {
  uint32_t stride, offset, block;
};
__host__ __device__ inline uint32_t seg_groups(uint32_t n_groups, QSeg q) {   // groups the segment owns
  const uint32_t cyc = q.block * q.stride, full = n_groups / cyc, rem = n_groups - full * cyc;
  const uint32_t lo = q.offset * q.block;
  return full * q.block + (rem > lo ? (rem - lo < q.block ? rem - lo : q.block) : 0u);
}
__host__ __device__ inline uint32_t seg_group(uint32_t unit, QSeg q) {        // the unit-th group of the segment
  return (unit / q.block) * (q.block * q.stride) + q.offset * q.block + unit % q.block;
}
__host__ __device__ inline bool seg_owns(uint32_t group, QSeg q) { return (group / q.block) % q.stride == q.offset; }
__host__ __device__ inline uint32_t seg_unit(uint32_t group, QSeg q) {        // (inverse of seg_group for an owned group)
  return (group / (q.block * q.stride)) * q.block + group % q.block;
}
// groups per block for n_segments segments (a constant: every rank derives the same deal; blocks of 4 .. 256 groups
// were measured at C3 and change nothing -- DESIGN.md 6)
constexpr uint32_t kSegBlockGroups = 1;
uint32_t seg_block(uint32_t n_segments);
// positions the padded orders of the pruned population sweeps add (dc_mfma_kernels.hpp: components padded to whole
// query groups: kMaxComp x kMaxGroupRows)
constexpr size_t kOrderPadRows = 64 * 512;
constexpr size_t kMinEdgeMaxRows = ((size_t)1 << 24) - kOrderPadRows;   // (the sweep's deferred-evaluation queue holds 24-bit positions)
// one Boruvka round on the radius graph (d2 < r2): for every component (d_comp[frame] = its id, any
// frame id) the lightest pair that leaves it, by (max(rank), min(rank)) with d_rank[frame] a
// permutation; d_best[id] = (max << 32 | min) or ~0.  d_pops: [n_rows] scratch (populations).
void launch_radius_min_edge(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2,
                            const uint32_t* d_comp, const uint32_t* d_rank, unsigned long long* d_best,
                            uint32_t* d_pops, void* d_ws, hipStream_t stream, uint32_t segment = 0,
                            uint32_t n_segments = 0);   // (n_segments > 0: the pairs seen from one segment's queries)
// neighbour sweep over (cell, free energy)-ordered frames with ring-wise pruning
// reuse_components: the component partition an earlier sweep over the same coordinates left in the workspace serves
// this one too (the second call of a populations -> neighbours pair); checked against a cookie on the device
void launch_nn_pruned(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe,
                      uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
                      uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t stream,
                      bool reuse_components = false);
// the same for one SEGMENT of the spatial order (segment s of n: a run of whole query groups): the
// rows a rank of a spatially sharded multi-GPU run answers for.  Outputs as for a row range: zeros /
// "none" for the rows of other segments.
void launch_pop_pruned_segment(const float* d_coords, uint32_t n_rows, uint32_t n_cols,
                               uint32_t segment, uint32_t n_segments, const Rad2& rad2, int n_rad,
                               uint32_t* d_pops_first_row, void* d_ws, hipStream_t stream, bool comp_clean = false);
void launch_nn_pruned_segment(const float* d_coords, uint32_t n_rows, uint32_t n_cols,
                              const float* d_fe, uint32_t segment, uint32_t n_segments,
                              uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2,
                              void* d_ws, hipStream_t stream, bool reuse_components = false);
void launch_nn_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe,
                    uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
                    uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t stream);

// cross sweeps (dc_hip_*_cross_dev), n_cols <= 64, every pair: the query rows [i_from, i_to) of d_query [n_q] against
// all n_ref >= 1 rows of d_ref, one origin and one scale over both sets.  Each call computes the statistics of both sets
// into the header first (the gated direct kernel reads its flag); pops [n_rad][n_q]; d_fe_q == nullptr: nn only.
// Return 0, or a negative code when a launch failed.
size_t cross_workspace_bytes(size_t n_q, size_t n_ref, size_t n_cols);
int launch_pop_cross_mfma(const float* d_query, uint32_t n_q, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                          uint32_t i_from, uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops, void* d_ws,
                          hipStream_t stream);
int launch_nn_cross_mfma(const float* d_query, uint32_t n_q, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                         const float* d_fe_q, const float* d_fe_r, uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx,
                         float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t stream);

// The rows of one segment of a sharded neighbour sweep compacted into a dense block [4][nn_block_rows] (nn_idx,
// nn_d2 bits, hd_idx, hd_d2 bits by local position), and the gathered blocks of all segments back to the four
// arrays by frame.  pruned: the segment sweep that ran was the pruned matrix-core sweep (its ordering is still in the
// workspace); otherwise, and for flagged data, the segments are the reference's row blocks.
size_t nn_block_rows(size_t n_rows, size_t n_cols, size_t n_segments);
void launch_nn_block_pack(const uint32_t* d_nn_idx, const float* d_nn_d2, const uint32_t* d_hd_idx,
                          const float* d_hd_d2, uint32_t n_rows, uint32_t n_cols, uint32_t segment,
                          uint32_t n_segments, bool pruned, const void* d_ws, uint32_t* d_block, hipStream_t stream);
void launch_nn_block_unpack(const uint32_t* d_blocks, uint32_t n_rows, uint32_t n_cols, uint32_t n_segments,
                            bool pruned, const void* d_ws, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                            float* d_hd_d2, hipStream_t stream);

// the frame pairs between ADJACENT components of a pruned population sweep (dc_mfma_kernels.hpp "components"), counted
// exactly and added to out[rr * stride + (query position | frame)]
void launch_pop_cross(const float* coords, uint32_t n_cols, const float* coords_r, const uint32_t* perm_r,
                      const float4* box_r, const uint32_t* perm_q, const float4* box_q, const uint32_t* tile_comp_q,
                      const uint32_t* comp, uint32_t T_q, uint32_t group_tiles, QSeg q_seg, int q_in_ref_order,
                      const Rad2& rad2, int n_rad, const uint32_t* hdr, uint32_t* out, size_t stride, int by_position,
                      hipStream_t s);

// diagnostics of the last pruned population sweep that ran in a workspace (synchronises): number of components, the
// global max |x - mean|^2, the bound of max |x - origin(component)|^2 the scale was chosen for, and that scale S
int components_info(const void* d_ws, size_t n_rows, size_t n_cols, uint32_t* n_comp, float* m_global, float* m_local,
                    float* scale, hipStream_t stream);

// Optional timing of the MAIN sweep kernels (bench.py's roofline entry wants the kernel's own duration, not the call's:
// the orderings and operand images are "prep").  When enabled the launchers bracket every main-kernel launch with HIP
// events on the launch stream: the first launch of a kind (0 population, 1 neighbour) since the last read sets the
// start, every launch moves the end.  sweep_timer_read synchronises on the end event.
void sweep_timer_enable(bool on);
void sweep_timer_mark(int kind, bool begin, hipStream_t s);
int sweep_timer_read(int kind, float* ms);   // 0 ok, -1 nothing recorded / error

// dc_sort.hip: stable key/value radix sort on the low key_bits bits of the keys (8 bits per pass).
// remap: the LAST pass writes the values only, into a padded order: the sorted list is cut into n_seg segments
// [seg_start[s], seg_start[s + 1]) (device arrays of n_seg + 1 entries; seg_start[n_seg] = n), segment s lands at
// positions seg_base[s] + 0, 1, ...; tags[position / 32] = s for every tile whose first position is taken.  Positions
// nothing lands on keep their contents (the caller presets them); keys_out is not written then.
constexpr uint32_t kSortMaxSegments = 64;
struct SortRemap {
  const uint32_t* seg_start;
  const uint32_t* seg_base;
  uint32_t n_seg;
  uint32_t* tags;
};
size_t sort_temp_bytes(size_t n);
// keys_in / vals_in are scratch: sorts of three or more passes use them for the passes in between.
int sort_pairs_u32(uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_in,
                   uint32_t* vals_out, size_t n, void* temp, size_t temp_bytes, hipStream_t stream,
                   unsigned key_bits = 32, const SortRemap* remap = nullptr);
constexpr unsigned kCellKeyBits = 24;   // cell keys of the spatial orderings: < 4002^2 < 2^24

}  // namespace dc
