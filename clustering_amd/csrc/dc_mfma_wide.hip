// dc_mfma_wide.hip -- host side of the matrix-core sweeps for rows of 65..256 columns: workspace, preparation and
// launches (kernels: dc_mfma_wide_kernels.hpp).
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

dim3 wide_grid(uint32_t i_from, uint32_t i_to, uint32_t Tp) {
  const uint32_t q_blocks = (i_to + kWideBlockRows - 1) / kWideBlockRows - i_from / kWideBlockRows;
  return dim3(wide_grid_size(q_blocks, wide_shares(Tp / kWideBlockTiles)));
}

// the counting sweep of the queries X.i_from .. X.i_to, for the rows of one array (kSelf) or against a reference
template <SweepMode SM>
void pop_wide(WideArgs X, const Rad2& rad2, int n_rad, uint32_t* d_pops_first_row, hipStream_t s) {
  X.rad2 = rad2;
  X.n_rad = n_rad;
  X.pops = d_pops_first_row;
  const dim3 grid = wide_grid(X.i_from, X.i_to, X.Tp);
  sweep_timer_mark(0, true, s);
  if (n_rad == 1)
    hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, 1, SM>), grid, dim3(256), 0, s, X);
  else if (n_rad <= 4)
    hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, 4, SM>), grid, dim3(256), 0, s, X);
  else
    hipLaunchKernelGGL((wide_sweep_kernel<kWidePop, kMaxRadiiPerLaunch, SM>), grid, dim3(256), 0, s, X);
  sweep_timer_mark(0, false, s);
}

// ... and the neighbour sweep (X.fe / X.q_fe set by the caller); n_q: the rows of the query array, whose merge words
// the sweep fills.  nn only: no word of the hd half is merged, so null hd outputs are never written.
template <SweepMode SM>
int nn_wide(const WideArgs& X, uint32_t n_q, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2,
            hipStream_t s) {
  if (hipMemsetAsync(X.merge, 0xFF, sizeof(unsigned long long) * 2 * (size_t)n_q, s) != hipSuccess) return -1;
  const dim3 grid = wide_grid(X.i_from, X.i_to, X.Tp);
  sweep_timer_mark(1, true, s);
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

}  // namespace dc
