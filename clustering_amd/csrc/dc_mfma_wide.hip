// dc_mfma_wide.hip -- host side of the matrix-core sweeps for rows of 65..256 columns: workspace, preparation and
// launches (kernels: dc_mfma_wide_kernels.hpp).  The unpruned self and cross sweeps also serve 257..1024 columns, in the
// layout of those widths (dc_hip_*_xwide_dev), and so do the pruned self population and neighbour sweeps
// (dc_hip_*_xwide_pruned_dev) and the pruned cross ones (dc_hip_*_cross_xwide_pruned_dev).
#include "dc_mfma_wide_kernels.hpp"

namespace dc {

size_t wide_workspace_bytes(size_t n_rows, size_t n_cols) {
  if (!wide_mfma_supports(n_cols) || n_rows == 0) return 0;
  return wide_layout(n_rows, n_cols).total;
}

size_t wide_against_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols) {
  if (!wide_mfma_supports(n_cols) || n_query == 0 || n_ref == 0) return 0;
  return wide_layout_against(n_query, n_ref, n_cols).total;
}

size_t xwide_workspace_bytes(size_t n_rows, size_t n_cols) {
  if (!xwide_mfma_supports(n_cols) || n_rows == 0) return 0;
  return wide_layout(n_rows, n_cols).total;
}

size_t xwide_against_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols) {
  if (!xwide_mfma_supports(n_cols) || n_query == 0 || n_ref == 0) return 0;
  return wide_layout_against(n_query, n_ref, n_cols).total;
}

namespace {

// The operands of a sweep in a workspace laid out by L: the reference side (a self sweep: all rows) in the fields the self
// sweep reads; a cross sweep adds its queries in the fields of their own, which a self sweep leaves zero
WideArgs wide_args(const WideLayout& L, const float* d_ref, uint32_t n_ref, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                   void* d_ws, const float* d_query = nullptr, uint32_t n_query = 0) {
  char* p = (char*)d_ws;
  WideArgs X{};
  X.coords = d_ref;
  X.n_rows = n_ref;
  X.n_cols = n_cols;
  X.NM = L.NM;
  X.Tp = L.Tp;
  X.img_a = (const uint4*)(p + L.off_img_a);
  X.img_b = (const uint4*)(p + L.off_img_b);
  X.norms = (const float*)(p + L.off_norms);
  X.hdr = (uint32_t*)p;
  X.i_from = i_from;
  X.i_to = i_to;
  X.merge = (unsigned long long*)(p + L.off_merge);
  X.q_coords = d_query;
  X.n_query = n_query;
  return X;
}

dim3 wide_grid(uint32_t i_from, uint32_t i_to, uint32_t Tp, WideGroup grp = kWideGroup88) {
  const uint32_t q_blocks = (i_to + kWideBlockRows - 1) / kWideBlockRows - i_from / kWideBlockRows;
  return dim3(wide_grid_size(q_blocks, wide_shares(Tp / kWideBlockTiles, grp), grp));
}

// The group of the unit map at 257..1024 columns: 8 x 8 like every other launch -- the smaller groups
// measured there were not faster by more than the spread of the runs, and moved no L2 hit rate.  -DDC_XWIDE_GROUP_Q=q -DDC_XWIDE_GROUP_S=s builds the unpruned instances of another shape
// for these widths, which is how that measurement was made (scratch/xwide_unit_ab.py); the default build holds none.
#ifndef DC_XWIDE_GROUP_Q
#define DC_XWIDE_GROUP_Q 8
#define DC_XWIDE_GROUP_S 8
#endif
constexpr WideGroup kXWideGroup{DC_XWIDE_GROUP_Q, DC_XWIDE_GROUP_S};
constexpr bool kXWideOwnGroup = kXWideGroup.gq != 8u || kXWideGroup.gs != 8u;
static_assert(kXWideGroup.gq >= 1 && kXWideGroup.gq <= 8 && (kXWideGroup.gq & (kXWideGroup.gq - 1)) == 0 && kXWideGroup.gs >= 1 &&
                  kXWideGroup.gs <= 8 && (kXWideGroup.gs & (kXWideGroup.gs - 1)) == 0,
              "a group: powers of two up to 8 x 8");

// the counting instance of a launch of n_rad radii -- one, up to four, up to kMaxRadiiPerLaunch --, timed as a population sweep
template <SweepMode SM, bool PR>
void launch_pop_instance(const WideKernelArgs<PR, false, PR && SM == kAgainst>& X, int n_rad, dim3 grid, hipStream_t s) {
  sweep_timer_mark(0, true, s);
  if (n_rad == 1)
    hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, 1, SM, PR>), grid, dim3(256), 0, s, X);
  else if (n_rad <= 4)
    hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, 4, SM, PR>), grid, dim3(256), 0, s, X);
  else
    hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, kMaxRadiiPerLaunch, SM, PR>), grid, dim3(256), 0, s, X);
  sweep_timer_mark(0, false, s);
}
// the largest fl32(r^2) of a launch: what the pruning rule of the pruned sweeps starts from
float largest_radius2(const Rad2& rad2, int n_rad) {
  float r2max = 0.0f;
  for (int k = 0; k < n_rad; ++k) r2max = rad2.v[k] > r2max ? rad2.v[k] : r2max;
  return r2max;
}
// a segment count as the kernels take it: clamped to 32 bits
uint32_t segments_u32(size_t n_segments) { return (uint32_t)(n_segments < 0xFFFFFFFFull ? n_segments : 0xFFFFFFFFull); }

// the counting sweep of the queries X.i_from .. X.i_to, for the rows of one array (kSelf) or against a reference
template <SweepMode SM>
void pop_wide(WideArgs X, const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row, hipStream_t s) {
  X.rad2 = rad2;
  X.n_rad = n_rad;
  X.pops = d_pops_first_row;
  if constexpr (kXWideOwnGroup) {
    if (X.n_cols > kWideMaxCols) {
      constexpr uint32_t Q = kXWideGroup.gq, S = kXWideGroup.gs;
      const dim3 grid = wide_grid(X.i_from, X.i_to, X.Tp, kXWideGroup);
      sweep_timer_mark(0, true, s);
      if (n_rad == 1)
        hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, 1, SM, false, Q, S>), grid, dim3(256), 0, s, X);
      else if (n_rad <= 4)
        hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, 4, SM, false, Q, S>), grid, dim3(256), 0, s, X);
      else
        hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, kMaxRadiiPerLaunch, SM, false, Q, S>), grid, dim3(256), 0, s, X);
      sweep_timer_mark(0, false, s);
      return;
    }
  }
  launch_pop_instance<SM, false>(X, n_rad, wide_grid(X.i_from, X.i_to, X.Tp), s);
}

// ... and the neighbour sweep (X.fe / X.q_fe set by the caller); n_q: the rows of the query array, whose merge words
// the sweep fills.  nn only: no word of the hd half is merged, so null hd outputs are never written.
template <SweepMode SM>
int nn_wide(const WideArgs& X, uint32_t n_q, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2,
            hipStream_t s) {
  if (hipMemsetAsync(X.merge, 0xFF, sizeof(unsigned long long) * 2 * (size_t)n_q, s) != hipSuccess) return -1;
  const bool own_group = kXWideOwnGroup && X.n_cols > kWideMaxCols;
  const dim3 grid = wide_grid(X.i_from, X.i_to, X.Tp, own_group ? kXWideGroup : kWideGroup88);
  sweep_timer_mark(1, true, s);
  if (own_group)
    hipLaunchKernelGGL((wide_sweep_kernel<kWideNn, 1, SM, false, kXWideGroup.gq, kXWideGroup.gs>), grid, dim3(256), 0, s, X);
  else
    hipLaunchKernelGGL((wide_sweep_kernel<kWideNn, 1, SM>), grid, dim3(256), 0, s, X);
  sweep_timer_mark(1, false, s);
  hipLaunchKernelGGL(wide_nn_finish_kernel, dim3((X.i_to - X.i_from + 255) / 256), dim3(256), 0, s, (const uint32_t*)X.hdr,
                     (const unsigned long long*)X.merge, n_q, X.i_from, X.i_to, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2);
  return 0;
}

}  // namespace

int wide_prepare(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, void* d_ws, hipStream_t s) {
  return wide_prepare_launches(d_coords, n_rows, n_cols, d_fe, d_ws, s);
}

void launch_pop_wide_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                          const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row, void* d_ws, hipStream_t s) {
  if (i_from >= i_to || n_rad <= 0) return;
  pop_wide<kSelf>(wide_args(wide_layout(n_rows, n_cols), d_coords, n_rows, n_cols, i_from, i_to, d_ws), rad2, n_rad,
                  d_pops_first_row, s);
}

int launch_nn_wide_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, uint32_t i_from,
                        uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws,
                        hipStream_t s) {
  if (i_from >= i_to) return 0;
  WideArgs X = wide_args(wide_layout(n_rows, n_cols), d_coords, n_rows, n_cols, i_from, i_to, d_ws);
  X.fe = d_fe;
  return nn_wide<kSelf>(X, n_rows, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, s);
}

// ---- the radius graph (dc_hip_radius_*_wide_dev): the one-radius self sweep with a sink --------------------
void launch_pairs_wide_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2, uint32_t* d_pops, uint2* d_pairs,
                            unsigned long long capacity, unsigned long long* d_count, void* d_ws, hipStream_t s) {
  if (n_rows == 0) return;
  WideArgs X = wide_args(wide_layout(n_rows, n_cols), d_coords, n_rows, n_cols, 0, n_rows, d_ws);
  X.rad2 = one_radius(r2);
  X.n_rad = 1;
  X.pops = d_pops;
  X.pairs = d_pairs;
  X.capacity = d_pairs ? capacity : 0ull;   // (counting only: every slot is beyond the list)
  X.count = d_count;
  sweep_timer_mark(0, true, s);
  hipLaunchKernelGGL((wide_sweep_kernel<kWidePairs, 1>), wide_grid(0, n_rows, X.Tp), dim3(256), 0, s, X);
  sweep_timer_mark(0, false, s);
}

void launch_min_edge_wide_mfma(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2, const uint32_t* d_comp,
                               const uint32_t* d_rank, uint32_t i_from, uint32_t i_to, unsigned long long* d_best,
                               uint32_t* d_pops, void* d_ws, hipStream_t s) {
  if (i_from >= i_to) return;
  WideArgs X = wide_args(wide_layout(n_rows, n_cols), d_coords, n_rows, n_cols, i_from, i_to, d_ws);
  X.rad2 = one_radius(r2);
  X.n_rad = 1;
  X.pops = d_pops;
  X.comp = d_comp;
  X.rank = d_rank;
  X.best = d_best;
  sweep_timer_mark(0, true, s);
  hipLaunchKernelGGL((wide_sweep_kernel<kWideMinEdge, 1>), wide_grid(i_from, i_to, X.Tp), dim3(256), 0, s, X);
  sweep_timer_mark(0, false, s);
}

// ---- the pruned self population sweep (dc_hip_populations_wide_pruned_dev) --------------------------------
namespace {
struct WidePrunedLayout {
  WideLayout L;      // the head: what the unpruned sweeps lay out
  uint32_t blocks;   // blocks of kWideBlockRows positions (= L.Tp / kWideBlockTiles)
  size_t off_perm, off_keys, off_keys_o, off_vals, off_coords, off_boxes, off_cnt, off_sort, sort_bytes, total;
};
WidePrunedLayout wide_pruned_layout(size_t n_rows, size_t n_cols) {
  WidePrunedLayout P;
  P.L = wide_layout(n_rows, n_cols);
  P.blocks = P.L.Tp / kWideBlockTiles;
  const size_t words = align256(sizeof(uint32_t) * n_rows);
  P.off_perm = P.L.total;   // [n_rows] position -> row
  P.off_keys = P.off_perm + words;
  P.off_keys_o = P.off_keys + words;
  P.off_vals = P.off_keys_o + words;
  P.off_coords = P.off_vals + words;   // [n_rows][n_cols] the rows in the order
  P.off_boxes = align256(P.off_coords + sizeof(float) * n_rows * n_cols);
  P.off_cnt = align256(P.off_boxes + sizeof(float4) * P.blocks);   // [kMaxRadiiPerLaunch][n_rows] counts by position
  P.off_sort = align256(P.off_cnt + sizeof(uint32_t) * kMaxRadiiPerLaunch * n_rows);
  P.sort_bytes = sort_temp_bytes(n_rows);
  P.total = align256(P.off_sort + P.sort_bytes);
  return P;
}
}  // namespace

size_t wide_pruned_workspace_bytes(size_t n_rows, size_t n_cols) {
  if (!wide_mfma_supports(n_cols) || n_rows == 0) return 0;
  return wide_pruned_layout(n_rows, n_cols).total;
}

// 257..1024 columns: the same regions behind the head of those widths.  wide_pruned_prepare,
// launch_pop_wide_pruned, launch_nn_wide_pruned and wide_pruned_order read the layout of the width they are given
size_t xwide_pruned_workspace_bytes(size_t n_rows, size_t n_cols) {
  if (!xwide_mfma_supports(n_cols) || n_rows == 0) return 0;
  return wide_pruned_layout(n_rows, n_cols).total;
}

int wide_pruned_prepare(const float* d_coords, uint32_t n_rows, uint32_t n_cols, void* d_ws, hipStream_t s, const float* d_fe) {
  const WidePrunedLayout P = wide_pruned_layout(n_rows, n_cols);
  char* p = (char*)d_ws;
  uint32_t* hdr = (uint32_t*)p;
  uint32_t* perm = (uint32_t*)(p + P.off_perm);
  uint32_t* keys = (uint32_t*)(p + P.off_keys);
  uint32_t* vals = (uint32_t*)(p + P.off_vals);
  float* coords_o = (float*)(p + P.off_coords);
  if (wide_stats_launches(d_coords, n_rows, n_cols, d_fe, d_ws, s) != 0) return -1;
  hipLaunchKernelGGL(wide_extent_kernel, dim3((uint32_t)min_sz(1024, ((size_t)n_rows + 255) / 256)), dim3(256), 0, s, d_coords,
                     n_rows, n_cols, hdr);
  hipLaunchKernelGGL(wide_prune_key_kernel, dim3((uint32_t)min_sz(4096, ((size_t)n_rows + 255) / 256)), dim3(256), 0, s, d_coords,
                     n_rows, n_cols, (const uint32_t*)hdr, keys, vals, n_rows, 0u);
  if (sort_pairs_u32(keys, (uint32_t*)(p + P.off_keys_o), vals, perm, n_rows, p + P.off_sort, P.sort_bytes, s, kCellKeyBits) != 0)
    return -1;
  hipLaunchKernelGGL(wide_prune_rows_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, s, d_coords, n_rows, n_cols,
                     (const uint32_t*)perm, P.blocks, coords_o, (float4*)(p + P.off_boxes), hdr + kWideHdrOrder, kWideOrderMark);
  return wide_image_launches(coords_o, n_rows, n_cols, d_ws, s);
}

namespace {
// the operands of a pruned launch of one chunk of radii over the query blocks segment, segment + n_segments, ... of the
// order, counting by position into row 0 of the count region (zeroed here); *grid: its workgroups
int wide_pruned_args(const WidePrunedLayout& P, uint32_t n_rows, uint32_t n_cols, size_t segment, size_t n_segments,
                     const Rad2& rad2, int n_rad, void* d_ws, hipStream_t s, WidePrunedArgs* out, dim3* grid) {
  char* p = (char*)d_ws;
  uint32_t* cnt = (uint32_t*)(p + P.off_cnt);
  if (hipMemsetAsync(cnt, 0, sizeof(uint32_t) * (size_t)n_rad * n_rows, s) != hipSuccess) return -1;
  WidePrunedArgs X{};
  static_cast<WideArgs&>(X) = wide_args(P.L, (const float*)(p + P.off_coords), n_rows, n_cols, 0, n_rows, d_ws);
  X.rad2 = rad2;
  X.n_rad = n_rad;
  X.pops = cnt;
  X.boxes = (const float4*)(p + P.off_boxes);
  X.seg = (uint32_t)segment;
  X.n_seg = segments_u32(n_segments);
  X.far2 = wide_prune_far2_at(largest_radius2(rad2, n_rad), n_cols);
  X.perm = (const uint32_t*)(p + P.off_perm);
  const uint32_t q_blocks = (uint32_t)((P.blocks - segment + n_segments - 1) / n_segments);
  *grid = dim3(wide_grid_size(q_blocks, wide_shares(P.blocks)));
  *out = X;
  return 0;
}
// counts by position -> populations by row, behind the sweep
int wide_pruned_scatter(const WidePrunedLayout& P, uint32_t n_rows, int n_rad, uint32_t* d_pops_first_row, void* d_ws, hipStream_t s) {
  char* p = (char*)d_ws;
  hipLaunchKernelGGL(wide_prune_scatter_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, s, (const uint32_t*)p,
                     (const uint32_t*)(p + P.off_perm), (const uint32_t*)(p + P.off_cnt), n_rows, n_rad, d_pops_first_row, n_rows);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace

int launch_pop_wide_pruned(uint32_t n_rows, uint32_t n_cols, size_t segment, size_t n_segments, const Rad2& rad2, int n_rad,
                           uint32_t* d_pops_first_row, void* d_ws, hipStream_t s) {
  if (n_rows == 0 || n_rad <= 0 || n_segments == 0) return 0;
  const WidePrunedLayout P = wide_pruned_layout(n_rows, n_cols);
  if (segment >= P.blocks) return 0;   // no block of the order: zeros (the caller's), no tile pair
  WidePrunedArgs X;
  dim3 grid;
  if (wide_pruned_args(P, n_rows, n_cols, segment, n_segments, rad2, n_rad, d_ws, s, &X, &grid) != 0) return -1;
  launch_pop_instance<kSelf, true>(X, n_rad, grid, s);
  return wide_pruned_scatter(P, n_rows, n_rad, d_pops_first_row, d_ws, s);
}

// ---- the pruned radius graph (dc_hip_radius_*_wide_pruned_dev): the pruned one-radius sweep with a sink ----
int launch_pairs_wide_pruned(uint32_t n_rows, uint32_t n_cols, float r2, uint32_t* d_pops, uint2* d_pairs,
                             unsigned long long capacity, unsigned long long* d_count, void* d_ws, hipStream_t s) {
  if (n_rows == 0) return 0;
  const WidePrunedLayout P = wide_pruned_layout(n_rows, n_cols);
  WidePrunedArgs X;
  dim3 grid;
  if (wide_pruned_args(P, n_rows, n_cols, 0, 1, one_radius(r2), 1, d_ws, s, &X, &grid) != 0) return -1;
  X.pairs = d_pairs;
  X.capacity = d_pairs ? capacity : 0ull;   // (counting only: every slot is beyond the list)
  X.count = d_count;
  sweep_timer_mark(0, true, s);
  hipLaunchKernelGGL((wide_sweep_kernel<kWidePairs, 1, kSelf, true>), grid, dim3(256), 0, s, X);
  sweep_timer_mark(0, false, s);
  return wide_pruned_scatter(P, n_rows, 1, d_pops, d_ws, s);
}

static_assert(kMaxRadiiPerLaunch >= 3, "rows 1 and 2 of the count region hold the gathered comp and rank of a one-radius call");
int launch_min_edge_wide_pruned(uint32_t n_rows, uint32_t n_cols, float r2, const uint32_t* d_comp, const uint32_t* d_rank,
                                size_t segment, size_t n_segments, unsigned long long* d_best, uint32_t* d_pops, void* d_ws,
                                hipStream_t s) {
  if (n_rows == 0 || n_segments == 0) return 0;
  const WidePrunedLayout P = wide_pruned_layout(n_rows, n_cols);
  if (segment >= P.blocks) return 0;   // no block of the order: nothing found (the caller's presets), no tile pair
  WidePrunedArgs X;
  dim3 grid;
  if (wide_pruned_args(P, n_rows, n_cols, segment, n_segments, one_radius(r2), 1, d_ws, s, &X, &grid) != 0) return -1;
  uint32_t* comp_o = X.pops + n_rows;
  uint32_t* rank_o = X.pops + 2 * (size_t)n_rows;
  hipLaunchKernelGGL(wide_prune_gather_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, s, X.perm, d_comp, d_rank, n_rows, comp_o,
                     rank_o);
  X.comp = comp_o;
  X.rank = rank_o;
  X.best = d_best;
  sweep_timer_mark(0, true, s);
  hipLaunchKernelGGL((wide_sweep_kernel<kWideMinEdge, 1, kSelf, true>), grid, dim3(256), 0, s, X);
  sweep_timer_mark(0, false, s);
  return wide_pruned_scatter(P, n_rows, 1, d_pops, d_ws, s);
}

// ---- the pruned self neighbour sweep (dc_hip_nearest_neighbors_wide_pruned_dev) ---------------------------
// Behind wide_pruned_prepare (with the free energies: a NaN among them flags the data).  The count region of the layout
// (32 bytes per row) holds, for this call, the free energies by position, then per block the (least, largest) free
// energy and the two bounds: 4 (n_rows + 1) + 16 blocks bytes, under 5 per row.  Three launches of the pruned neighbour
// instance -- seed, ring 1, ring 2 (dc_wide_prune.hpp) --, the bounds kernel in front of the second and the third, the
// finish kernel behind them; the counters add up over the launches.
int launch_nn_wide_pruned(const float* d_fe, uint32_t n_rows, uint32_t n_cols, size_t segment, size_t n_segments,
                          uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t s) {
  if (n_rows == 0 || n_segments == 0) return 0;
  const WidePrunedLayout P = wide_pruned_layout(n_rows, n_cols);
  if (segment >= P.blocks) return 0;   // no block of the order: "none" everywhere (the caller's preset), no tile pair
  char* p = (char*)d_ws;
  const size_t off_range = P.off_cnt + sizeof(float) * (((size_t)n_rows + 1) & ~(size_t)1);
  const size_t off_far2 = off_range + sizeof(float2) * P.blocks;
  static_assert(sizeof(uint32_t) * kMaxRadiiPerLaunch >= 24, "one row: 8 bytes of free energies and 16 of its block fit the count region");
  float* fe_o = (float*)(p + P.off_cnt);
  float2* fe_range = (float2*)(p + off_range);
  float* far2 = (float*)(p + off_far2);   // [2][blocks]: nn, hd
  WideNnPrunedArgs X{};
  static_cast<WideArgs&>(X) = wide_args(P.L, (const float*)(p + P.off_coords), n_rows, n_cols, 0, n_rows, d_ws);
  X.fe = fe_o;
  X.boxes = (const float4*)(p + P.off_boxes);
  X.seg = (uint32_t)segment;
  X.n_seg = segments_u32(n_segments);
  X.perm = (const uint32_t*)(p + P.off_perm);
  X.far2_nn = far2;
  X.far2_hd = far2 + P.blocks;
  X.fe_range = fe_range;
  if (hipMemsetAsync(X.merge, 0xFF, sizeof(unsigned long long) * 2 * (size_t)n_rows, s) != hipSuccess) return -1;
  hipLaunchKernelGGL(wide_nn_gather_kernel, dim3(P.blocks), dim3(128), 0, s, X.perm, d_fe, n_rows, fe_o, fe_range);
  const uint32_t q_blocks = (uint32_t)((P.blocks - segment + n_segments - 1) / n_segments);
  const dim3 grid(wide_grid_size(q_blocks, wide_shares(P.blocks)));
  sweep_timer_mark(1, true, s);
  for (uint32_t ring = kWideRingSeed; ring <= kWideRing2; ++ring) {
    if (ring != kWideRingSeed)
      hipLaunchKernelGGL(wide_nn_bounds_kernel, dim3(P.blocks), dim3(128), 0, s, (const unsigned long long*)X.merge, n_rows,
                         ring - 1u, far2 + (size_t)(ring - 1u) * P.blocks, wide_nn_floor(n_cols));
    X.ring = ring;
    hipLaunchKernelGGL((wide_sweep_kernel<kWideNn, 1, kSelf, true>), grid, dim3(256), 0, s, X);
  }
  sweep_timer_mark(1, false, s);
  hipLaunchKernelGGL(wide_nn_finish_pruned_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, s, (const uint32_t*)p,
                     (const unsigned long long*)X.merge, X.perm, n_rows, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the counters of the last sweep back to zero: a further round in a prepared workspace reports its own
int wide_clear_counters(void* d_ws, hipStream_t s) {
  static_assert(kWideHdrMfma == kWideHdrTiles + 2 && kWideHdrExact == kWideHdrTiles + 4, "three 64-bit counters side by side");
  return hipMemsetAsync((char*)d_ws + 4 * kWideHdrTiles, 0, 24, s) == hipSuccess ? 0 : -1;
}

int wide_pruned_order(const void* d_ws, uint32_t n_rows, uint32_t n_cols, uint32_t* d_perm, hipStream_t s) {
  uint32_t tag[3] = {0u, 0u, 0u};
  if (hipMemcpyAsync(tag, (const char*)d_ws + 4 * kWideHdrOrder, sizeof(tag), hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
  if (hipStreamSynchronize(s) != hipSuccess) return -1;
  if (tag[0] != kWideOrderMark || tag[1] != n_rows || tag[2] != n_cols) return 1;
  const WidePrunedLayout P = wide_pruned_layout(n_rows, n_cols);
  if (hipMemcpyAsync(d_perm, (const char*)d_ws + P.off_perm, sizeof(uint32_t) * (size_t)n_rows, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return -1;
  return 0;
}

// ---- neighbour blocks of a sharded run in the order of the pruned sweep (dc_hip_neighbors_block_*_wide_dev) --
// Segment g of G owns the query blocks g, g + G, ... of the order; by LOCAL POSITION l its rows form a dense block an
// all-gather can move: local block l / 128 is block (l / 128) G + g of the order, position p(l), row perm[p].  Flagged
// data (the direct kernel answered on the reference's row block) uses the row block: chosen on the device from header
// word 1, the word the sweep's gate read.  The layout header -- the last kWideBlockHdrRows entries of plane 0 -- says under
// which layout a block was packed: mark | by position, positions, block size, segment count, deal (1: block b goes to
// segment b mod G), and the 64-bit hash of the order.
namespace {
constexpr uint32_t kWideBlockHdrRows = 32, kWideBlockHdrWords = 7, kWideBlockMagic = 0x6E6E5700u;   // "nnW" | by_position
constexpr uint32_t kWideBlockNoOrder = 2u;   // ... | the workspace holds no order of this shape: nothing packed, never unpacked

__device__ __forceinline__ uint32_t wide_block_none(uint32_t c, uint32_t n_rows) {
  return (c & 1u) ? __float_as_uint(FLT_MAX) : n_rows + 1u;
}
// 0: row blocks (flagged data), 1: by position, kWideBlockNoOrder: unflagged, but no order of n_rows x n_cols is signed
__device__ __forceinline__ uint32_t wide_block_mode(const uint32_t* __restrict__ hdr, uint32_t n_rows, uint32_t n_cols) {
  if (hdr[1] != 0u) return 0u;
  const bool signed_here = hdr[kWideHdrOrder] == kWideOrderMark && hdr[kWideHdrOrder + 1] == n_rows && hdr[kWideHdrOrder + 2] == n_cols;
  return signed_here ? 1u : kWideBlockNoOrder;
}
// word k < kWideBlockHdrWords of the header this workspace packs under
__device__ __forceinline__ uint32_t wide_block_hdr_word(uint32_t k, uint32_t mode, const uint32_t* __restrict__ hdr, uint32_t n_rows,
                                                        uint32_t G) {
  const bool by_position = mode == 1u;
  switch (k) {
    case 0: return kWideBlockMagic | mode;
    case 1: return n_rows;   // positions of the order (it has no pads) = rows of the row blocks
    case 2: return by_position ? kWideBlockRows : 0u;
    case 3: return G;
    case 4: return by_position ? 1u : 0u;
    case 5: return by_position ? hdr[kWideHdrOrderHash] : 0u;
    case 6: return by_position ? hdr[kWideHdrOrderHash + 1] : 0u;
    default: return 0u;
  }
}
// wrap-around sum over the positions of a mixed (position, row) word: the same for every launch shape
__global__ __launch_bounds__(256) void wide_order_hash_kernel(const uint32_t* __restrict__ perm, uint32_t n_rows,
                                                              unsigned long long* __restrict__ hash) {
  unsigned long long acc = 0ull;
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n_rows; p += gridDim.x * 256u) {
    unsigned long long x = (((unsigned long long)p << 32) | perm[p]) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    acc += x ^ (x >> 32);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63u) == 0 && acc != 0ull) atomicAdd(hash, acc);
}
__global__ __launch_bounds__(256) void wide_block_pack_kernel(const uint32_t* __restrict__ nn_idx, const float* __restrict__ nn_d2,
                                                              const uint32_t* __restrict__ hd_idx, const float* __restrict__ hd_d2,
                                                              uint32_t n_rows, uint32_t n_cols, uint32_t seg, uint32_t G,
                                                              uint32_t block_rows, const uint32_t* __restrict__ perm,
                                                              const uint32_t* __restrict__ hdr, uint32_t* __restrict__ block) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l >= block_rows) return;
  const uint32_t mode = wide_block_mode(hdr, n_rows, n_cols);
  const uint32_t payload = block_rows - kWideBlockHdrRows;
  if (l >= payload) {
    const uint32_t k = l - payload;
    block[l] = k < kWideBlockHdrWords ? wide_block_hdr_word(k, mode, hdr, n_rows, G) : 0u;
    for (uint32_t c = 1; c < 4; ++c) block[c * (size_t)block_rows + l] = wide_block_none(c, n_rows);
    return;
  }
  uint32_t i = 0xFFFFFFFFu;
  if (mode == 1u) {
    const unsigned long long p = ((unsigned long long)(l / kWideBlockRows) * G + seg) * kWideBlockRows + l % kWideBlockRows;
    if (p < n_rows) i = perm[p];
  } else if (mode == 0u) {
    const uint32_t rng = n_rows / G, lo = seg * rng, hi = (seg == G - 1u) ? n_rows : lo + rng;
    if (l < hi - lo) i = lo + l;
  }
  const bool live = i < n_rows;
  block[0 * (size_t)block_rows + l] = live ? nn_idx[i] : wide_block_none(0, n_rows);
  block[1 * (size_t)block_rows + l] = live ? __float_as_uint(nn_d2[i]) : wide_block_none(1, n_rows);
  block[2 * (size_t)block_rows + l] = live ? hd_idx[i] : wide_block_none(2, n_rows);
  block[3 * (size_t)block_rows + l] = live ? __float_as_uint(hd_d2[i]) : wide_block_none(3, n_rows);
}
// Every workgroup compares the G headers with the one this workspace packs under before it scatters anything: on a
// mismatch nothing is written; workgroup 0 records the verdict of THIS unpack (dc_hip_wide_layout_status_dev).
__global__ __launch_bounds__(256) void wide_block_unpack_kernel(const uint32_t* __restrict__ blocks /* [G][4][block_rows] */,
                                                                uint32_t n_rows, uint32_t n_cols, uint32_t G, uint32_t block_rows,
                                                                const uint32_t* __restrict__ perm, uint32_t* __restrict__ hdr,
                                                                uint32_t* __restrict__ nn_idx, float* __restrict__ nn_d2,
                                                                uint32_t* __restrict__ hd_idx, float* __restrict__ hd_d2) {
  __shared__ uint32_t bad_s;
  if (threadIdx.x == 0) bad_s = 0u;
  __syncthreads();
  const uint32_t mode = wide_block_mode(hdr, n_rows, n_cols);
  const uint32_t payload = block_rows - kWideBlockHdrRows;
  if (mode == kWideBlockNoOrder && threadIdx.x == 0) bad_s = 1u;
  for (uint32_t e = threadIdx.x; e < kWideBlockHdrWords * G; e += 256u) {
    const uint32_t r = e / kWideBlockHdrWords, k = e - kWideBlockHdrWords * r;
    if (blocks[(size_t)r * 4u * block_rows + payload + k] != wide_block_hdr_word(k, mode, hdr, n_rows, G)) bad_s = 1u;
  }
  __syncthreads();
  const uint32_t bad = bad_s;
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr[kWideHdrLayoutBad] = bad;
  if (bad != 0u) return;
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_rows) return;
  uint32_t i, r, l;
  if (mode == 1u) {
    const uint32_t b = p / kWideBlockRows;
    r = b % G;
    l = (b / G) * kWideBlockRows + p % kWideBlockRows;
    i = perm[p];
    if (i >= n_rows) return;
  } else {
    const uint32_t rng = n_rows / G;
    i = p;
    r = rng ? min(p / rng, G - 1u) : G - 1u;
    l = p - r * rng;
  }
  const uint32_t* b = blocks + (size_t)r * 4u * block_rows;
  nn_idx[i] = b[l];
  nn_d2[i] = __uint_as_float(b[(size_t)block_rows + l]);
  hd_idx[i] = b[2 * (size_t)block_rows + l];
  hd_d2[i] = __uint_as_float(b[3 * (size_t)block_rows + l]);
}
// the hash of the order the workspace holds, into its header (the sum starts from zero)
int wide_order_hash(void* d_ws, uint32_t n_rows, uint32_t n_cols, hipStream_t s) {
  const WidePrunedLayout P = wide_pruned_layout(n_rows, n_cols);
  char* p = (char*)d_ws;
  unsigned long long* hash = (unsigned long long*)(p + 4 * kWideHdrOrderHash);
  if (hipMemsetAsync(hash, 0, sizeof(unsigned long long), s) != hipSuccess) return -1;
  hipLaunchKernelGGL(wide_order_hash_kernel, dim3((uint32_t)min_sz(1024, ((size_t)n_rows + 255) / 256)), dim3(256), 0, s,
                     (const uint32_t*)(p + P.off_perm), n_rows, hash);
  return 0;
}
}  // namespace

namespace {
// rows of a block of n_rows rows dealt to n_segments (both positive): no function of the width
size_t nn_block_rows_of(size_t n_rows, size_t n_segments) {
  const size_t row_block = n_rows - (n_segments - 1) * (n_rows / n_segments);   // the last (largest) row block
  const size_t blocks = (n_rows + kWideBlockRows - 1) / kWideBlockRows;
  const size_t most = (blocks + n_segments - 1) / n_segments;   // segment 0 owns the most blocks of the order
  const size_t by_position = most * kWideBlockRows;
  return (row_block > by_position ? row_block : by_position) + kWideBlockHdrRows;
}
}  // namespace

size_t wide_nn_block_rows(size_t n_rows, size_t n_cols, size_t n_segments) {
  if (!wide_mfma_supports(n_cols) || n_segments == 0 || n_rows == 0) return 0;
  return nn_block_rows_of(n_rows, n_segments);
}

// 257..1024 columns: the same blocks; the launchers below read the layout of the width they are given
size_t xwide_nn_block_rows(size_t n_rows, size_t n_cols, size_t n_segments) {
  if (!xwide_mfma_supports(n_cols) || n_segments == 0 || n_rows == 0) return 0;
  return nn_block_rows_of(n_rows, n_segments);
}

int launch_nn_block_pack_wide(const uint32_t* d_nn_idx, const float* d_nn_d2, const uint32_t* d_hd_idx, const float* d_hd_d2,
                              uint32_t n_rows, uint32_t n_cols, uint32_t segment, uint32_t n_segments, void* d_ws, uint32_t* d_block,
                              hipStream_t s) {
  const uint32_t rows = (uint32_t)nn_block_rows_of(n_rows, n_segments);   // (either family: the caller checked the width)
  if (wide_order_hash(d_ws, n_rows, n_cols, s) != 0) return -1;
  const char* p = (const char*)d_ws;
  hipLaunchKernelGGL(wide_block_pack_kernel, dim3((rows + 255u) / 256u), dim3(256), 0, s, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, n_rows,
                     n_cols, segment, n_segments, rows, (const uint32_t*)(p + wide_pruned_layout(n_rows, n_cols).off_perm),
                     (const uint32_t*)p, d_block);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_nn_block_unpack_wide(const uint32_t* d_blocks, uint32_t n_rows, uint32_t n_cols, uint32_t n_segments, void* d_ws,
                                uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, hipStream_t s) {
  const uint32_t rows = (uint32_t)nn_block_rows_of(n_rows, n_segments);   // (either family: the caller checked the width)
  if (wide_order_hash(d_ws, n_rows, n_cols, s) != 0) return -1;
  char* p = (char*)d_ws;
  hipLaunchKernelGGL(wide_block_unpack_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, s, d_blocks, n_rows, n_cols, n_segments,
                     rows, (const uint32_t*)(p + wide_pruned_layout(n_rows, n_cols).off_perm), (uint32_t*)p, d_nn_idx, d_nn_d2,
                     d_hd_idx, d_hd_d2);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int wide_layout_status(const void* d_ws, int* mismatch, hipStream_t s) {
  uint32_t w = 0;
  if (hipMemcpyAsync(&w, (const char*)d_ws + 4 * kWideHdrLayoutBad, sizeof(w), hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
  if (hipStreamSynchronize(s) != hipSuccess) return -1;
  *mismatch = w != 0u ? 1 : 0;
  return 0;
}

int wide_prepare_against(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                         void* d_ws, hipStream_t s) {
  return wide_prepare_against_launches(d_query, n_query, d_ref, n_ref, n_cols, d_ws, s);
}

void launch_pop_wide_against(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                             uint32_t i_from, uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row,
                             void* d_ws, hipStream_t s) {
  if (i_from >= i_to || n_rad <= 0 || n_ref == 0) return;
  pop_wide<kAgainst>(wide_args(wide_layout_against(n_query, n_ref, n_cols), d_ref, n_ref, n_cols, i_from, i_to, d_ws, d_query,
                               n_query),
                     rad2, n_rad, d_pops_first_row, s);
}

int launch_nn_wide_against(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                           const float* d_fe_query, const float* d_fe_ref, uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx,
                           float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t s) {
  if (i_from >= i_to || n_ref == 0) return 0;
  WideArgs X = wide_args(wide_layout_against(n_query, n_ref, n_cols), d_ref, n_ref, n_cols, i_from, i_to, d_ws, d_query, n_query);
  X.q_fe = d_fe_query;
  X.fe = d_fe_query ? d_fe_ref : nullptr;
  return nn_wide<kAgainst>(X, n_query, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, s);
}

// ---- the pruned cross population sweep (dc_hip_populations_cross_wide_pruned_dev) -------------------------
namespace {
struct WideCrossPrunedLayout {
  WideLayout L;                  // the head: what the unpruned cross sweeps lay out for n_query x n_ref
  uint32_t blocks_r, blocks_q;   // blocks of kWideBlockRows positions: the reference's, the whole query array's
  size_t off_perm_r, off_perm_q, off_keys, off_keys_o, off_vals, off_coords_r, off_coords_q, off_boxes_r, off_boxes_q, off_cnt,
      off_sort, sort_bytes, total;
};
WideCrossPrunedLayout wide_cross_pruned_layout(size_t n_query, size_t n_ref, size_t n_cols) {
  WideCrossPrunedLayout P;
  P.L = wide_layout_against(n_query, n_ref, n_cols);
  P.blocks_r = P.L.Tp / kWideBlockTiles;
  P.blocks_q = P.L.Tqp / kWideBlockTiles;
  const size_t n_max = n_query > n_ref ? n_query : n_ref;
  const size_t words_r = align256(sizeof(uint32_t) * n_ref), words_q = align256(sizeof(uint32_t) * n_query);
  const size_t words = align256(sizeof(uint32_t) * n_max);
  P.off_perm_r = P.L.total;                 // [n_ref] position -> row of the reference
  P.off_perm_q = P.off_perm_r + words_r;    // [i_to - i_from] position -> row of the query array
  P.off_keys = P.off_perm_q + words_q;      // keys and values of one sort: the reference's, then the query range's
  P.off_keys_o = P.off_keys + words;
  P.off_vals = P.off_keys_o + words;
  P.off_coords_r = P.off_vals + words;      // [n_ref][n_cols] the reference in its order
  P.off_coords_q = align256(P.off_coords_r + sizeof(float) * n_ref * n_cols);   // [i_to - i_from][n_cols] the queries in theirs
  P.off_boxes_r = align256(P.off_coords_q + sizeof(float) * n_query * n_cols);
  P.off_boxes_q = align256(P.off_boxes_r + sizeof(float4) * P.blocks_r);
  P.off_cnt = align256(P.off_boxes_q + sizeof(float4) * P.blocks_q);   // [kMaxRadiiPerLaunch][i_to - i_from] counts by query position
  P.off_sort = align256(P.off_cnt + sizeof(uint32_t) * kMaxRadiiPerLaunch * n_query);
  P.sort_bytes = sort_temp_bytes(n_max);
  P.total = align256(P.off_sort + P.sort_bytes);
  return P;
}
}  // namespace

size_t wide_cross_pruned_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols) {
  if (!wide_mfma_supports(n_cols) || n_query == 0 || n_ref == 0) return 0;
  return wide_cross_pruned_layout(n_query, n_ref, n_cols).total;
}

// 257..1024 columns: the same regions behind the head of those widths.  wide_cross_pruned_prepare,
// launch_pop_wide_cross_pruned, launch_nn_wide_cross_pruned and wide_cross_pruned_order read the layout of the width they
// are given
size_t xwide_cross_pruned_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols) {
  if (!xwide_mfma_supports(n_cols) || n_query == 0 || n_ref == 0) return 0;
  return wide_cross_pruned_layout(n_query, n_ref, n_cols).total;
}

int wide_cross_pruned_prepare(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols,
                              uint32_t i_from, uint32_t i_to, void* d_ws, hipStream_t s) {
  const WideCrossPrunedLayout P = wide_cross_pruned_layout(n_query, n_ref, n_cols);
  const uint32_t n_q = i_to - i_from;
  char* p = (char*)d_ws;
  uint32_t* hdr = (uint32_t*)p;
  uint32_t* keys = (uint32_t*)(p + P.off_keys);
  uint32_t* keys_o = (uint32_t*)(p + P.off_keys_o);
  uint32_t* vals = (uint32_t*)(p + P.off_vals);
  const float* q_range = d_query + (size_t)i_from * n_cols;
  // one origin, one scale, M over every row of both arrays: the statistics of the unpruned cross sweep
  if (wide_stats_against_launches(d_query, n_query, d_ref, n_ref, n_cols, d_ws, s) != 0) return -1;
  if (hipMemsetD32Async((hipDeviceptr_t)(hdr + kWideHdrOrderLaidOut), (int)n_query, 1, s) != hipSuccess) return -1;
  // one grid for both sets: the extent of the query range and the reference together, the cell from the reference's count
  struct Side {
    const float* rows;      // the first row a position can name ...
    uint32_t n, row0;       // ... how many there are, and the number of the first in its array
    const float* array;     // the array perm's rows index
    size_t off_perm, off_coords, off_boxes;
    uint32_t sign, mark;
  } const sides[2] = {{d_ref, n_ref, 0u, d_ref, P.off_perm_r, P.off_coords_r, P.off_boxes_r, kWideHdrOrderRef, kWideOrderMarkRef},
                      {q_range, n_q, i_from, d_query, P.off_perm_q, P.off_coords_q, P.off_boxes_q, kWideHdrOrderQuery, kWideOrderMarkQuery}};
  for (const Side& side : sides)
    hipLaunchKernelGGL(wide_extent_kernel, dim3((uint32_t)min_sz(1024, ((size_t)side.n + 255) / 256)), dim3(256), 0, s, side.rows,
                       side.n, n_cols, hdr);
  for (const Side& side : sides) {
    uint32_t* perm = (uint32_t*)(p + side.off_perm);
    hipLaunchKernelGGL(wide_prune_key_kernel, dim3((uint32_t)min_sz(4096, ((size_t)side.n + 255) / 256)), dim3(256), 0, s, side.rows,
                       side.n, n_cols, (const uint32_t*)hdr, keys, vals, n_ref, side.row0);
    if (sort_pairs_u32(keys, keys_o, vals, perm, side.n, p + P.off_sort, P.sort_bytes, s, kCellKeyBits) != 0) return -1;
    hipLaunchKernelGGL(wide_prune_rows_kernel, dim3((side.n + 255u) / 256u), dim3(256), 0, s, side.array, side.n, n_cols,
                       (const uint32_t*)perm, (side.n + kWideBlockRows - 1u) / kWideBlockRows, (float*)(p + side.off_coords),
                       (float4*)(p + side.off_boxes), hdr + side.sign, side.mark);
  }
  return wide_image_against_launches(P.L, (const float*)(p + P.off_coords_q), n_q, (const float*)(p + P.off_coords_r), n_ref,
                                     n_cols, d_ws, s);
}

namespace {
// the launch in a workspace whose places P names: the n_q gathered query rows against the gathered reference, the counts
// scattered to rows of a population array of n_query rows per radius
int pop_wide_cross_pruned(const WideCrossPrunedLayout& P, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t n_q,
                          const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row, void* d_ws, hipStream_t s) {
  char* p = (char*)d_ws;
  uint32_t* cnt = (uint32_t*)(p + P.off_cnt);
  if (hipMemsetAsync(cnt, 0, sizeof(uint32_t) * (size_t)n_rad * n_q, s) != hipSuccess) return -1;
  WideCrossPrunedArgs X{};
  static_cast<WideArgs&>(X) = wide_args(P.L, (const float*)(p + P.off_coords_r), n_ref, n_cols, 0, n_q, d_ws,
                                        (const float*)(p + P.off_coords_q), n_q);
  X.rad2 = rad2;
  X.n_rad = n_rad;
  X.pops = cnt;
  X.boxes = (const float4*)(p + P.off_boxes_r);
  X.qboxes = (const float4*)(p + P.off_boxes_q);
  X.seg = 0;
  X.n_seg = 1;
  X.far2 = wide_prune_far2_at(largest_radius2(rad2, n_rad), n_cols);   // (up to 256 columns: no floor)
  launch_pop_instance<kAgainst, true>(X, n_rad, dim3(wide_grid_size((n_q + kWideBlockRows - 1u) / kWideBlockRows, wide_shares(P.blocks_r))),
                                      s);
  hipLaunchKernelGGL(wide_prune_scatter_kernel, dim3((n_q + 255u) / 256u), dim3(256), 0, s, (const uint32_t*)p,
                     (const uint32_t*)(p + P.off_perm_q), (const uint32_t*)cnt, n_q, n_rad, d_pops_first_row, n_query);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace

int launch_pop_wide_cross_pruned(uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                                 const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row, void* d_ws, hipStream_t s) {
  if (i_from >= i_to || n_rad <= 0 || n_ref == 0) return 0;
  return pop_wide_cross_pruned(wide_cross_pruned_layout(n_query, n_ref, n_cols), n_query, n_ref, n_cols, i_to - i_from, rad2, n_rad,
                               d_pops_first_row, d_ws, s);
}

// ---- the pruned cross neighbour sweep (dc_hip_nearest_neighbors_cross_wide_pruned_dev) --------------------
// Behind wide_cross_pruned_prepare in the same workspace.  The sort's keys, keys_o and vals arrays (n_max words each) are
// free once both orders stand: the first two hold the free energies of the reference and of the query range by position,
// the third the words per block -- fe_min per reference block, then fe_max, far2_nn, far2_hd and the seed per query
// block: blocks_r + 4 blocks_q <= 5 ceil(n_max / 128) words, inside n_max words from n_max = 6 on and inside the 256
// bytes of align256 below.  A NaN free energy of either side flags the data (ring 2 rests on the ranges per block): the
// gathers raise header word 1 on the stream, before the first sweep launch.  Then the launches of 4.24: seed, bounds, ring 1, bounds, ring 2, finish.
namespace {
// where the free-energy words of a neighbour sweep lie: the free energies of either side by position, the least per
// reference block, and [4][P.blocks_q] words per query block -- the largest free energy, far2 nn, far2 hd, the seed
struct WideCrossNnPlaces {
  size_t off_fe_r, off_fe_q, off_fe_min_r, off_qwords;
  size_t off_flag_q;     // the header word a NaN among the queries' free energies raises (bytes)
  bool ref_resident;     // the reference's words stand (the resident reference gathered them when they were set)
};
// the launches in a workspace whose places P and N name: the n_q gathered query rows against the gathered reference
int nn_wide_cross_pruned(const WideCrossPrunedLayout& P, const WideCrossNnPlaces& N, uint32_t n_ref, uint32_t n_cols, uint32_t n_q,
                         const float* d_fe_query, const float* d_fe_ref, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                         float* d_hd_d2, void* d_ws, hipStream_t s) {
  const uint32_t blocks_q = (n_q + kWideBlockRows - 1u) / kWideBlockRows;
  char* p = (char*)d_ws;
  float* fe_r = (float*)(p + N.off_fe_r);
  float* fe_q = (float*)(p + N.off_fe_q);
  float* fe_min_r = (float*)(p + N.off_fe_min_r);   // [blocks_r]
  float* fe_max_q = (float*)(p + N.off_qwords);     // [blocks_q of the whole query array] each from here on
  float* far2 = fe_max_q + P.blocks_q;              // [2]: nn, hd
  uint32_t* seed = (uint32_t*)(far2 + 2 * (size_t)P.blocks_q);
  WideCrossNnPrunedArgs X{};
  static_cast<WideArgs&>(X) = wide_args(P.L, (const float*)(p + P.off_coords_r), n_ref, n_cols, 0, n_q, d_ws,
                                        (const float*)(p + P.off_coords_q), n_q);
  X.boxes = (const float4*)(p + P.off_boxes_r);
  X.qboxes = (const float4*)(p + P.off_boxes_q);
  X.seg = 0;
  X.n_seg = 1;
  X.perm = (const uint32_t*)(p + P.off_perm_r);
  X.far2_nn = far2;
  X.far2_hd = far2 + P.blocks_q;
  X.fe_min_r = fe_min_r;
  X.fe_max_q = fe_max_q;
  X.seed = seed;
  const uint32_t* perm_q = (const uint32_t*)(p + P.off_perm_q);
  if (hipMemsetAsync(X.merge, 0xFF, sizeof(unsigned long long) * 2 * (size_t)n_q, s) != hipSuccess) return -1;
  if (d_fe_query) {
    // (the gathers and the seed kernel run on flagged data too: they read through the two orders and the boxes, which
    //  wide_cross_pruned_prepare completes whatever the rows hold -- a preparation that stood down on flagged data would
    //  have to gate them)
    if (!N.ref_resident)
      hipLaunchKernelGGL(wide_cross_nn_gather_kernel, dim3(P.blocks_r), dim3(128), 0, s, X.perm, d_fe_ref, n_ref, 0u, fe_r, fe_min_r,
                         (uint32_t*)p + 1);
    hipLaunchKernelGGL(wide_cross_nn_gather_kernel, dim3(blocks_q), dim3(128), 0, s, perm_q, d_fe_query, n_q, 1u, fe_q, fe_max_q,
                       (uint32_t*)(p + N.off_flag_q));
    X.fe = fe_r;
    X.q_fe = fe_q;
  }
  // (the resident reference: word 1 of this sweep from its flags, those of the free energies just gathered among them)
  if (N.ref_resident) hipLaunchKernelGGL(wide_res_arm_kernel, dim3(1), dim3(64), 0, s, (uint32_t*)p, d_fe_query ? 1u : 0u);
  hipLaunchKernelGGL(wide_cross_seed_kernel, dim3(blocks_q), dim3(64), 0, s, X.qboxes, X.boxes, P.blocks_r, seed);
  const dim3 grid(wide_grid_size(blocks_q, wide_shares(P.blocks_r)));
  const uint32_t last_ring = d_fe_query ? kWideRing2 : kWideRing1;   // no ring 2 without free energies
  sweep_timer_mark(1, true, s);
  for (uint32_t ring = kWideRingSeed; ring <= last_ring; ++ring) {
    if (ring != kWideRingSeed)
      hipLaunchKernelGGL(wide_nn_bounds_kernel, dim3(blocks_q), dim3(128), 0, s, (const unsigned long long*)X.merge, n_q, ring - 1u,
                         far2 + (size_t)(ring - 1u) * P.blocks_q, wide_nn_floor(n_cols));
    X.ring = ring;
    hipLaunchKernelGGL((wide_sweep_kernel<kWideNn, 1, kAgainst, true>), grid, dim3(256), 0, s, X);
  }
  sweep_timer_mark(1, false, s);
  hipLaunchKernelGGL(wide_nn_finish_pruned_kernel, dim3((n_q + 255u) / 256u), dim3(256), 0, s, (const uint32_t*)p,
                     (const unsigned long long*)X.merge, perm_q, n_q, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace

int launch_nn_wide_cross_pruned(uint32_t n_query, uint32_t n_ref, uint32_t n_cols, const float* d_fe_query, const float* d_fe_ref,
                                uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                float* d_hd_d2, void* d_ws, hipStream_t s) {
  if (i_from >= i_to || n_ref == 0) return 0;
  const WideCrossPrunedLayout P = wide_cross_pruned_layout(n_query, n_ref, n_cols);
  const WideCrossNnPlaces N{P.off_keys, P.off_keys_o, P.off_vals, P.off_vals + sizeof(float) * P.blocks_r, 4, false};
  return nn_wide_cross_pruned(P, N, n_ref, n_cols, i_to - i_from, d_fe_query, d_fe_ref, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, d_ws, s);
}

int wide_cross_pruned_order(const void* d_ws, uint32_t n_query_range, uint32_t n_ref, uint32_t n_cols, uint32_t* d_perm_q,
                            uint32_t* d_perm_r, hipStream_t s) {
  uint32_t tag[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  static_assert(kWideHdrOrderQuery == kWideHdrOrderRef + 3 && kWideHdrOrderLaidOut == kWideHdrOrderRef + 6, "seven words side by side");
  if (hipMemcpyAsync(tag, (const char*)d_ws + 4 * kWideHdrOrderRef, sizeof(tag), hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
  if (hipStreamSynchronize(s) != hipSuccess) return -1;
  if (tag[0] != kWideOrderMarkRef || tag[1] != n_ref || tag[2] != n_cols || tag[3] != kWideOrderMarkQuery ||
      tag[4] != n_query_range || tag[5] != n_cols || tag[6] < n_query_range)
    return 1;
  const WideCrossPrunedLayout P = wide_cross_pruned_layout(tag[6], n_ref, n_cols);
  if (hipMemcpyAsync(d_perm_q, (const char*)d_ws + P.off_perm_q, sizeof(uint32_t) * (size_t)n_query_range, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(d_perm_r, (const char*)d_ws + P.off_perm_r, sizeof(uint32_t) * (size_t)n_ref, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return -1;
  return 0;
}

// ---- the resident reference of the pruned cross sweeps (dc_hip_reference_wide_*; at 257..1024 columns
// ---- dc_hip_reference_xwide_*, 4.36: the same functions in the layout of that width) ------------------------------------
// The preparation of wide_cross_pruned_prepare in two halves: the reference's, once, under statistics that do not depend
// on a batch (dc_mfma_wide_kernels.hpp, "the resident reference"), and a batch's.  The sweeps are launch_pop_wide_cross_pruned
// and launch_nn_wide_cross_pruned as they stand, in a workspace of three regions:
//   resident (n_ref, n_cols):    A image, norms, the reference's order, its gathered rows, its boxes; its free energies by
//                                position, their least per block, and a copy by row for the direct kernel
//   batch (max_batch, n_cols):   B image, merge words, the batch's order, its gathered rows, its boxes, the counts; the
//                                queries' free energies by position and the four words per query block
//   scratch (the larger count):  keys, sorted keys, values and the sort's own bytes -- the reference's sort once, then a
//                                batch's; nothing that outlives a sort lies here
namespace {
struct WideReferenceLayout {
  WideCrossPrunedLayout P;   // the places of the pruned cross sweep (P.L: the images, norms and merge words)
  WideCrossNnPlaces N;       // ... and of its free-energy words
  size_t off_fe_row;         // [n_ref] the reference's free energies by row
  size_t resident_begin, resident_end, batch_begin, batch_end;   // scratch: batch_end .. P.total
};
WideReferenceLayout wide_reference_layout(size_t n_ref, size_t n_cols, size_t max_batch) {
  WideReferenceLayout R;
  WideCrossPrunedLayout& P = R.P;
  WideLayout& L = P.L;
  L.T = (uint32_t)((n_ref + 31) / 32);
  L.Tp = wide_pad_tiles(L.T);
  L.Tq = (uint32_t)((max_batch + 31) / 32);
  L.Tqp = wide_pad_tiles(L.Tq);
  L.NM = (uint32_t)nm_for((int)n_cols);
  P.blocks_r = L.Tp / kWideBlockTiles;
  P.blocks_q = L.Tqp / kWideBlockTiles;
  const size_t tile_bytes = (size_t)16 * 64 * L.NM;
  const size_t n_max = max_batch > n_ref ? max_batch : n_ref;
  size_t at = wide_off_images(n_cols);   // (up to 256 columns kWideOffImages; beyond, behind [1024] sums and means)
  auto take = [&at](size_t bytes) {
    const size_t off = at;
    at = align256(at + bytes);
    return off;
  };
  R.resident_begin = at;
  L.off_img_a = take(tile_bytes * L.Tp);
  L.off_norms = take(sizeof(float) * 32 * (size_t)L.Tp);
  P.off_perm_r = take(sizeof(uint32_t) * n_ref);
  P.off_coords_r = take(sizeof(float) * n_ref * n_cols);
  P.off_boxes_r = take(sizeof(float4) * P.blocks_r);
  R.N.off_fe_r = take(sizeof(float) * n_ref);
  R.N.off_fe_min_r = take(sizeof(float) * P.blocks_r);
  R.off_fe_row = take(sizeof(float) * n_ref);
  R.resident_end = R.batch_begin = at;
  L.off_img_b = take(tile_bytes * L.Tqp);
  L.off_merge = take(sizeof(unsigned long long) * 2 * max_batch);
  P.off_perm_q = take(sizeof(uint32_t) * max_batch);
  P.off_coords_q = take(sizeof(float) * max_batch * n_cols);
  P.off_boxes_q = take(sizeof(float4) * P.blocks_q);
  P.off_cnt = take(sizeof(uint32_t) * kMaxRadiiPerLaunch * max_batch);
  R.N.off_fe_q = take(sizeof(float) * max_batch);
  R.N.off_qwords = take(sizeof(uint32_t) * 4 * P.blocks_q);
  R.batch_end = at;
  P.off_keys = take(sizeof(uint32_t) * n_max);
  P.off_keys_o = take(sizeof(uint32_t) * n_max);
  P.off_vals = take(sizeof(uint32_t) * n_max);
  P.sort_bytes = sort_temp_bytes(n_max);
  P.off_sort = take(P.sort_bytes);
  P.total = L.total = at;
  R.N.off_flag_q = 4 * kWideHdrResFlagFeQuery;
  R.N.ref_resident = true;
  return R;
}
// one side's rows in the workspace's grid order: sort by the keys in the scratch, gather, box, sign
int wide_reference_order(const WideReferenceLayout& R, const float* d_rows, uint32_t n, uint32_t n_cols, size_t off_perm,
                         size_t off_coords, size_t off_boxes, uint32_t sign, uint32_t mark, void* d_ws, hipStream_t s) {
  char* p = (char*)d_ws;
  uint32_t* perm = (uint32_t*)(p + off_perm);
  if (sort_pairs_u32((uint32_t*)(p + R.P.off_keys), (uint32_t*)(p + R.P.off_keys_o), (uint32_t*)(p + R.P.off_vals), perm, n,
                     p + R.P.off_sort, R.P.sort_bytes, s, kCellKeyBits) != 0)
    return -1;
  hipLaunchKernelGGL(wide_prune_rows_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, d_rows, n, n_cols, (const uint32_t*)perm,
                     (n + kWideBlockRows - 1u) / kWideBlockRows, (float*)(p + off_coords), (float4*)(p + off_boxes),
                     (uint32_t*)p + sign, mark);
  return 0;
}
}  // namespace

size_t wide_reference_workspace_bytes(size_t n_ref, size_t n_cols, size_t max_batch) {
  if (!wide_mfma_supports(n_cols) || n_ref == 0 || max_batch == 0) return 0;
  return wide_reference_layout(n_ref, n_cols, max_batch).P.total;
}
// ... and of the third kind (dc_hip_reference_xwide_*): rows of 257..1024 columns.  Every other function of
// the resident form reads the layout of the width it is given, as wide_cross_pruned_prepare does, and serves both kinds.
size_t xwide_reference_workspace_bytes(size_t n_ref, size_t n_cols, size_t max_batch) {
  if (!xwide_mfma_supports(n_cols) || n_ref == 0 || max_batch == 0) return 0;
  return wide_reference_layout(n_ref, n_cols, max_batch).P.total;
}

int wide_reference_open(const float* d_ref, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, void* d_ws, hipStream_t s) {
  const WideReferenceLayout R = wide_reference_layout(n_ref, n_cols, max_batch);
  char* p = (char*)d_ws;
  uint32_t* hdr = (uint32_t*)p;
  float* means = (float*)(p + wide_off_means(n_cols));
  // statistics of the reference alone (wide_stats_launches without the free energies and with the resident scale)
  if (hipMemsetAsync(d_ws, 0, wide_off_images(n_cols), s) != hipSuccess) return -1;
  const size_t elems = (size_t)n_ref * n_cols;
  hipLaunchKernelGGL(wide_colsum_kernel, dim3((uint32_t)min_sz(1024, (elems + 255) / 256)), dim3(256), 0, s, d_ref, n_ref, n_cols,
                     (double*)(p + kWideOffSums));
  hipLaunchKernelGGL(wide_mean_kernel, dim3(1), dim3(256), 0, s, (const double*)(p + kWideOffSums), (size_t)n_ref, n_cols,
                     means);
  hipLaunchKernelGGL(wide_rowstats_kernel, dim3((uint32_t)min_sz(4096, ((size_t)n_ref + 3) / 4)), dim3(256), 0, s, d_ref, n_ref,
                     n_cols, (const float*)means, hdr);
  hipLaunchKernelGGL(wide_res_scale_kernel, dim3(1), dim3(1), 0, s, hdr);
  if (hipMemsetD32Async((hipDeviceptr_t)(hdr + kWideHdrOrderLaidOut), (int)max_batch, 1, s) != hipSuccess) return -1;
  // the grid: the reference's extent, the cell from its count; its order, gathered rows, boxes, A image and norms
  hipLaunchKernelGGL(wide_extent_kernel, dim3((uint32_t)min_sz(1024, ((size_t)n_ref + 255) / 256)), dim3(256), 0, s, d_ref, n_ref,
                     n_cols, hdr);
  hipLaunchKernelGGL(wide_prune_key_kernel, dim3((uint32_t)min_sz(4096, ((size_t)n_ref + 255) / 256)), dim3(256), 0, s, d_ref, n_ref,
                     n_cols, (const uint32_t*)hdr, (uint32_t*)(p + R.P.off_keys), (uint32_t*)(p + R.P.off_vals), n_ref, 0u);
  if (wide_reference_order(R, d_ref, n_ref, n_cols, R.P.off_perm_r, R.P.off_coords_r, R.P.off_boxes_r, kWideHdrOrderRef,
                           kWideOrderMarkRef, d_ws, s) != 0)
    return -1;
  const WideLayout& L = R.P.L;
  const size_t frags = (size_t)L.Tp * L.NM * 64;
  hipLaunchKernelGGL(wide_image_kernel, dim3((uint32_t)((frags + 255) / 256)), dim3(256), 0, s, (const float*)(p + R.P.off_coords_r),
                     n_ref, n_cols, L.NM, L.Tp, (const float*)means, (const uint32_t*)p, (uint4*)(p + L.off_img_a), (uint4*)nullptr,
                     (float*)(p + L.off_norms));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int wide_reference_set_free_energies(const float* d_fe_ref, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, void* d_ws,
                                     hipStream_t s) {
  const WideReferenceLayout R = wide_reference_layout(n_ref, n_cols, max_batch);
  char* p = (char*)d_ws;
  uint32_t* hdr = (uint32_t*)p;
  float* fe_row = (float*)(p + R.off_fe_row);
  if (hipMemcpyAsync(fe_row, d_fe_ref, sizeof(float) * (size_t)n_ref, hipMemcpyDeviceToDevice, s) != hipSuccess) return -1;
  if (hipMemsetD32Async((hipDeviceptr_t)(hdr + kWideHdrResFlagFeRef), 0, 1, s) != hipSuccess) return -1;
  hipLaunchKernelGGL(wide_cross_nn_gather_kernel, dim3(R.P.blocks_r), dim3(128), 0, s, (const uint32_t*)(p + R.P.off_perm_r),
                     (const float*)fe_row, n_ref, 0u, (float*)(p + R.N.off_fe_r), (float*)(p + R.N.off_fe_min_r),
                     hdr + kWideHdrResFlagFeRef);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

const float* wide_reference_fe_by_row(const void* d_ws, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch) {
  return (const float*)((const char*)d_ws + wide_reference_layout(n_ref, n_cols, max_batch).off_fe_row);
}

int wide_reference_stage(const float* d_query, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, void* d_ws,
                         hipStream_t s) {
  const WideReferenceLayout R = wide_reference_layout(n_ref, n_cols, max_batch);
  char* p = (char*)d_ws;
  uint32_t* hdr = (uint32_t*)p;
  const float* means = (const float*)(p + wide_off_means(n_cols));
  hipLaunchKernelGGL(wide_res_batch_reset_kernel, dim3(1), dim3(64), 0, s, hdr);
  if (n_query == 0) return hipGetLastError() == hipSuccess ? 0 : -1;
  // the gate: four columns per lane up to 256 columns, sixteen beyond
  const dim3 gate_grid((uint32_t)min_sz(4096, ((size_t)n_query + 3) / 4));
  uint32_t* keys = (uint32_t*)(p + R.P.off_keys);
  uint32_t* vals = (uint32_t*)(p + R.P.off_vals);
  if (n_cols <= kWideMaxCols)
    hipLaunchKernelGGL(wide_res_gate_kernel<kWideGateSlots>, gate_grid, dim3(256), 0, s, d_query, n_query, n_cols, means, hdr, keys,
                       vals, n_ref);
  else
    hipLaunchKernelGGL(wide_res_gate_kernel<kXWideGateSlots>, gate_grid, dim3(256), 0, s, d_query, n_query, n_cols, means, hdr, keys,
                       vals, n_ref);
  if (wide_reference_order(R, d_query, n_query, n_cols, R.P.off_perm_q, R.P.off_coords_q, R.P.off_boxes_q, kWideHdrOrderQuery,
                           kWideOrderMarkQuery, d_ws, s) != 0)
    return -1;
  const WideLayout& L = R.P.L;
  const uint32_t Tqp = wide_pad_tiles((n_query + 31u) / 32u);
  const size_t frags = (size_t)Tqp * L.NM * 64;
  hipLaunchKernelGGL(wide_image_kernel, dim3((uint32_t)((frags + 255) / 256)), dim3(256), 0, s, (const float*)(p + R.P.off_coords_q),
                     n_query, n_cols, L.NM, Tqp, means, (const uint32_t*)p, (uint4*)nullptr, (uint4*)(p + L.off_img_b), (float*)nullptr);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int wide_reference_arm(void* d_ws, hipStream_t s) {
  hipLaunchKernelGGL(wide_res_arm_kernel, dim3(1), dim3(64), 0, s, (uint32_t*)d_ws, 0u);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pop_wide_reference(uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, const Rad2& rad2, int n_rad,
                              uint32_t* d_pops_first_row, void* d_ws, hipStream_t s) {
  if (n_query == 0 || n_rad <= 0) return 0;
  return pop_wide_cross_pruned(wide_reference_layout(n_ref, n_cols, max_batch).P, n_query, n_ref, n_cols, n_query, rad2, n_rad,
                               d_pops_first_row, d_ws, s);
}

int launch_nn_wide_reference(uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch, const float* d_fe_query,
                             uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, hipStream_t s) {
  if (n_query == 0) return 0;
  const WideReferenceLayout R = wide_reference_layout(n_ref, n_cols, max_batch);
  if (hipMemsetD32Async((hipDeviceptr_t)((uint32_t*)d_ws + kWideHdrResFlagFeQuery), 0, 1, s) != hipSuccess) return -1;
  return nn_wide_cross_pruned(R.P, R.N, n_ref, n_cols, n_query, d_fe_query, nullptr, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, d_ws, s);
}

int wide_reference_info(const void* d_ws, uint64_t* tiles, uint64_t* mfmas, uint64_t* exact_pairs, uint32_t* answered, hipStream_t s) {
  uint32_t h[kWideHdrResAnswered + 1];
  if (hipMemcpyAsync(h, d_ws, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
  if (hipStreamSynchronize(s) != hipSuccess) return -1;
  if (tiles) *tiles = ((uint64_t)h[kWideHdrTiles + 1] << 32) | h[kWideHdrTiles];
  if (mfmas) *mfmas = ((uint64_t)h[kWideHdrMfma + 1] << 32) | h[kWideHdrMfma];
  if (exact_pairs) *exact_pairs = ((uint64_t)h[kWideHdrExact + 1] << 32) | h[kWideHdrExact];
  if (answered) *answered = h[kWideHdrResAnswered];
  return 0;
}

int wide_reference_order_copy(const void* d_ws, uint32_t n_query, uint32_t n_ref, uint32_t n_cols, uint32_t max_batch,
                              uint32_t* d_perm_q, uint32_t* d_perm_r, hipStream_t s) {
  const WideReferenceLayout R = wide_reference_layout(n_ref, n_cols, max_batch);
  const char* p = (const char*)d_ws;
  if (d_perm_q && n_query &&
      hipMemcpyAsync(d_perm_q, p + R.P.off_perm_q, sizeof(uint32_t) * (size_t)n_query, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return -1;
  if (d_perm_r && hipMemcpyAsync(d_perm_r, p + R.P.off_perm_r, sizeof(uint32_t) * (size_t)n_ref, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return -1;
  return hipStreamSynchronize(s) == hipSuccess ? 0 : -1;
}

}  // namespace dc
