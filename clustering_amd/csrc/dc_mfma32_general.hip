// dc_mfma32_general.hip -- the fp32-input MFMA sweeps (dc_mfma32.hpp) for rows of 1..32 columns and up to 8 radii per
// pass of the MFMAs: the kernel instances, their planner and their launchers (dc_hip_*_fp32_dev).  A
// unit of its own, as dc_mfma_step.hip is, so that dc_mfma.hip keeps its compile time; the two orders of the sweeps
// (mfma32_order_pop / _nn) stay with the sort plumbing in dc_mfma.hip.
//
// Instances: S = 1, 3, 5, ..., 15 and 16 K-steps.  S = ceil(D / 2) is exact for D = 1, 2, 5, 6, 9, 10, ..., 29, 30 (the
// widths of BASELINE.json's five configurations: 5, 10, 30) and for D = 31, 32; the other widths run one zero K-step
// more (fp32_steps).  The band (guard_eps32, scale32_pop) is evaluated with K = 2 S of the INSTANCE -- a zero step adds
// nothing to the chain, the bound only grows.
#include "dc_mfma_kernels.hpp"
#include "dc_mfma32_band.hpp"

#include <algorithm>
#include <cassert>

namespace dc {

namespace {

#include "dc_mfma32.hpp"

// query tiles per wave: what the 256 registers of __launch_bounds__(256, 2) hold beside b[TQ][S], the two fragment sets,
// the two sets of row norms and four accumulator tiles (the table); the several-radii kernel keeps
// what it has per radius in LDS; its call of pop32_multi_chain asks for more of the registers a call preserves, so it
// takes four query tiles from S = 5 on and clumps of two chains from S = 11 on
constexpr int tq_pop32(int S, int n_rad) { return (S <= 3 || (S <= 5 && n_rad <= 1)) ? 8 : 4; }
constexpr int clump_pop32(int S) { return S <= 9 ? kClump32 : 2; }
constexpr int tq_nn32(int S) { return S <= 5 ? 4 : 2; }

struct Pop32Args {
  const float* coords;
  uint32_t n_rows, n_cols;
  const float *img, *norms;
  const uint32_t *perm, *hdr;
  uint32_t T, i_from, i_to;
  float r2max;
  uint32_t wpb, env_chunks;
};

// dynamic LDS of a population workgroup, and its waves: DC_MFMA32_WPB, halved until the workgroup's LDS stays within the
// 64 KB a kernel gets without asking (the counts of 8 radii x 8 query tiles are 16 KB per wave)
inline uint32_t pop32_smem(uint32_t wpb, int tq, int n_rad) {
  return wpb * (uint32_t)sizeof(float) * (n_rad <= 1 ? 2u * kNormBatch32 * 32u : pop32m_wave_words(tq, n_rad));
}
inline uint32_t pop32_wpb(uint32_t wpb, int tq, int n_rad) {
  while (wpb > 1 && pop32_smem(wpb, tq, n_rad) > 64u * 1024u) wpb /= 2;
  return wpb;
}
inline uint32_t pop32_chunks(const Pop32Args& A, int tq, uint32_t wpb, uint32_t* blocks) {
  *blocks = ((A.T + tq - 1) / tq + wpb - 1) / wpb;   // (all positions: the rows of a range are scattered over the order)
  return A.env_chunks ? std::min(A.env_chunks, A.T) : chunks32(*blocks * wpb, A.T, 2048u);
}

// one sweep of n_rad <= 8 radii; pops: [n_rad][n_rows]
template <int S>
void pop32_sweep(const Pop32Args& A, const Rad2& rad2, int n_rad, uint32_t* pops, hipStream_t stream) {
  constexpr int kTQ1 = tq_pop32(S, 1), kTQm = tq_pop32(S, 2);
  const int tq = n_rad == 1 ? kTQ1 : kTQm;
  const uint32_t wpb = pop32_wpb(A.wpb, tq, n_rad);
  uint32_t blocks = 0;
  const uint32_t chunks = pop32_chunks(A, tq, wpb, &blocks);
  const dim3 grid(blocks, chunks), block(64 * wpb);
  const size_t smem = pop32_smem(wpb, tq, n_rad);
  if (chunks > 1)
    for (int r = 0; r < n_rad; ++r)
      (void)hipMemsetAsync(pops + (size_t)r * A.n_rows + A.i_from, 0, sizeof(uint32_t) * (size_t)(A.i_to - A.i_from), stream);
  sweep_timer_mark(0, true, stream);
  if (n_rad == 1)
    hipLaunchKernelGGL((pop_mfma32_kernel<S, kTQ1>), grid, block, smem, stream, A.coords, A.n_rows, A.n_cols, A.img, A.norms, A.perm,
                       A.hdr, A.T, A.i_from, A.i_to, rad2.v[0], A.r2max, pops);
  else
    hipLaunchKernelGGL((pop_mfma32_multi_kernel<S, kTQm, clump_pop32(S)>), grid, block, smem, stream, A.coords, A.n_rows, A.n_cols, A.img, A.norms,
                       A.perm, A.hdr, A.T, A.i_from, A.i_to, rad2, n_rad, A.r2max, pops);
  sweep_timer_mark(0, false, stream);
}

struct Nn32Args {
  const float* coords;
  uint32_t n_rows, n_cols;
  const float *img, *norms, *img_s, *norms_s;
  const uint32_t *perm, *invpos, *pq, *hdr;
  uint32_t T, i_from, i_to;
  unsigned long long* merge64;
  uint32_t *nn_idx, *hd_idx;
  float *nn_d2, *hd_d2;
  uint32_t blocks, chunks, wpb, smem;
};

template <int S>
void nn32_sweep(const Nn32Args& A, hipStream_t stream) {
  hipLaunchKernelGGL((nn_mfma32_kernel<S, tq_nn32(S)>), dim3(A.blocks, A.chunks), dim3(64 * A.wpb), A.smem, stream, A.coords, A.n_rows,
                     A.n_cols, A.img, A.norms, A.img_s, A.norms_s, A.perm, A.invpos, A.pq, A.hdr, A.T, A.i_from, A.i_to, A.merge64,
                     A.nn_idx, A.nn_d2, A.hd_idx, A.hd_d2);
}

#define DC_FP32_INSTANCES(X) X(1) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(16)

// waves per workgroup of the neighbour sweep: DC_MFMA32_WPB, halved until the workgroup's LDS stays within the 64 KB a
// kernel gets without asking (at most 4 waves x 22 KB today: the rule is there for the day a wave's share grows)
inline uint32_t nn32_smem(uint32_t wpb, uint32_t tq, uint32_t n_cols) {
  return wpb * (uint32_t)sizeof(uint32_t) * (2 * kNormBatch32 * 32 + 2 * kWaveQueue + 4 * tq * 32 + tq * 32 * n_cols);
}
inline uint32_t nn32_wpb(uint32_t tq, uint32_t n_cols) {
  uint32_t wpb = sweep_switches().mfma32_wpb;
  while (wpb > 1 && nn32_smem(wpb, tq, n_cols) > 64u * 1024u) wpb /= 2;
  return wpb;
}

}  // namespace

bool fp32_supports(size_t n_cols) { return n_cols >= 1 && n_cols <= kFp32MaxCols; }

uint32_t fp32_steps(size_t n_cols) {
  const uint32_t s = (uint32_t)steps32((int)n_cols);
  return (s % 2 == 0 && s < 16) ? s + 1 : s;
}

Fp32Plan fp32_plan(size_t n_rows, size_t n_cols, size_t n_radii) {
  assert(n_rows >= 1 && fp32_supports(n_cols) && n_radii >= 1);
  const Layout L = make_layout(n_rows, n_cols);
  Fp32Plan P{};
  P.steps = fp32_steps(n_cols);
  P.lane_floats = (uint32_t)lane32((int)P.steps);
  // (measured at 100 000 rows of 10 and of 30 columns for every count from 2 to 8, profiles/fp32_general_ab.json cases
  //  k10 / k30: one pass for the radii of a call is faster than a pass per radius at each -- the closest is two radii at
  //  10 columns, where the query tiles per wave drop from 8 to 4: 3.33 against 4.04 ms -- so no count is routed through
  //  the per-radius loop)
  P.radii_per_sweep = (uint32_t)std::min<size_t>(n_radii, kMaxRadiiPerLaunch);
  P.sweeps = (uint32_t)((n_radii + P.radii_per_sweep - 1) / P.radii_per_sweep);
  P.tq_pop = (uint32_t)tq_pop32((int)P.steps, (int)P.radii_per_sweep);
  P.tq_nn = (uint32_t)tq_nn32((int)P.steps);
  const SweepSwitches& sw = sweep_switches();
  Pop32Args A{};
  A.T = L.T;
  A.wpb = sw.mfma32_wpb;
  A.env_chunks = sw.mfma32_chunks;
  uint32_t blocks = 0;
  const uint32_t wpb_pop = pop32_wpb(A.wpb, (int)P.tq_pop, (int)P.radii_per_sweep);
  P.chunks_pop = pop32_chunks(A, (int)P.tq_pop, wpb_pop, &blocks);
  const uint32_t wpb_nn = nn32_wpb(P.tq_nn, (uint32_t)n_cols);
  const uint32_t blocks_nn = (grid_for(0, (uint32_t)n_rows, (int)P.tq_nn) * 4u + wpb_nn - 1) / wpb_nn;
  P.chunks_nn = sw.mfma32_chunks ? std::min(sw.mfma32_chunks, L.T) : chunks32(blocks_nn * wpb_nn, L.T, 2048u);
  P.lds_pop = pop32_smem(wpb_pop, (int)P.tq_pop, (int)P.radii_per_sweep);
  P.lds_nn = nn32_smem(wpb_nn, P.tq_nn, (uint32_t)n_cols);
  P.image_bytes = 64u * P.lane_floats * (uint32_t)sizeof(float);
  // what make_layout keeps per tile for an operand image (16 B x 64 lanes per MFMA of the fp16 x 2 form) and, per row, for
  // a norm; the norms ring reads up to 15 tiles past the last one: the pad tiles of the padded orders
  P.region_bytes = 16u * 64u * L.NM;
  assert(P.image_bytes <= P.region_bytes && "fp32 operand image larger than the layout's image region");
  assert((size_t)P.image_bytes * L.T <= L.off_img_b - L.off_img && sizeof(float) * 32 * ((size_t)L.T + 16) <= L.off_img_s - L.off_norm);
  return P;
}

void launch_pop_fp32(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                     const float* rad2_all, size_t n_radii, uint32_t* d_pops, void* d_ws, hipStream_t stream) {
  const Layout L = make_layout(n_rows, n_cols);
  const Fp32Plan P = fp32_plan(n_rows, n_cols, n_radii);
  char* p = (char*)d_ws;
  float* img = (float*)(p + L.off_img);
  float* norms = (float*)(p + L.off_norm);
  if (mfma32_order_pop(d_coords, n_rows, n_cols, d_ws, stream) != 0) return;
  // (ONE image for all radii of the call, scaled for the largest: the band of a smaller radius is narrower than 1)
  float r2max = 0.0f;
  for (size_t r = 0; r < n_radii; ++r) r2max = std::max(r2max, rad2_all[r]);
  hipLaunchKernelGGL(image32_kernel, dim3((32 * L.T + 255) / 256), dim3(256), 0, stream, d_coords, n_rows, n_cols, L.T,
                     (const float*)(p + kHdrMeans), (const uint32_t*)(p + L.off_perm), (const uint32_t*)p, r2max, P.steps, sweep_switches().mfma32_poison_pads,
                     img, norms);
  const SweepSwitches& sw = sweep_switches();
  const Pop32Args A{d_coords, n_rows, n_cols, img, norms, (const uint32_t*)(p + L.off_perm), (const uint32_t*)p, L.T, i_from, i_to,
                    r2max, sw.mfma32_wpb, sw.mfma32_chunks};
  for (size_t r0 = 0; r0 < n_radii; r0 += P.radii_per_sweep) {
    const int n_rad = (int)std::min<size_t>(P.radii_per_sweep, n_radii - r0);
    Rad2 rad2;
    for (int r = 0; r < kMaxRadiiPerLaunch; ++r) rad2.v[r] = (r < n_rad) ? rad2_all[r0 + r] : -1.0f;
    uint32_t* out = d_pops + r0 * n_rows;
    switch (P.steps) {
#define X_(SV) case SV: pop32_sweep<SV>(A, rad2, n_rad, out, stream); break;
      DC_FP32_INSTANCES(X_)
#undef X_
      default: assert(!"no fp32 instance for this K-step count");
    }
  }
}

void launch_nn_fp32(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, uint32_t i_from,
                    uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws,
                    hipStream_t stream) {
  // (launch_nn_mfma32's steps: natural-order image for the queries, the frames by free energy, their image)
  const Layout L = make_layout(n_rows, n_cols);
  const uint32_t steps = fp32_steps(n_cols);
  char* p = (char*)d_ws;
  const dim3 blk(256), grid_t((32 * L.T + 255) / 256);
  float* img = (float*)(p + L.off_img);
  float* norms = (float*)(p + L.off_norm);
  float* img_s = (float*)(p + L.off_img_s);
  float* norms_s = (float*)(p + L.off_norm_s);
  const uint32_t* perm = (const uint32_t*)(p + L.off_perm);
  hipLaunchKernelGGL(image32_kernel, grid_t, blk, 0, stream, d_coords, n_rows, n_cols, L.T, (const float*)(p + kHdrMeans),
                     (const uint32_t*)nullptr, (const uint32_t*)p, -1.0f, steps, sweep_switches().mfma32_poison_pads, img, norms);
  if (mfma32_order_nn(n_rows, n_cols, d_fe, d_ws, stream) != 0) return;
  hipLaunchKernelGGL(image32_kernel, grid_t, blk, 0, stream, d_coords, n_rows, n_cols, L.T, (const float*)(p + kHdrMeans), perm,
                     (const uint32_t*)p, -1.0f, steps, sweep_switches().mfma32_poison_pads, img_s, norms_s);
  const uint32_t env_chunks = sweep_switches().mfma32_chunks;
  const uint32_t tq = (uint32_t)tq_nn32((int)steps), wpb = nn32_wpb(tq, n_cols);
  const uint32_t blocks = (grid_for(i_from, i_to, (int)tq) * 4u + wpb - 1) / wpb;
  const uint32_t chunks = env_chunks ? std::min(env_chunks, L.T) : chunks32(blocks * wpb, L.T, 2048u);
  unsigned long long* merge64 = (unsigned long long*)(p + L.off_merge64);
  if (chunks > 1)
    hipLaunchKernelGGL(nn_merge_fill_kernel, dim3((2 * n_rows + 255) / 256), dim3(256), 0, stream, merge64, n_rows);
  const Nn32Args A{d_coords, n_rows, n_cols, img, norms, img_s, norms_s, perm, (const uint32_t*)(p + L.off_invpos),
                   (const uint32_t*)(p + L.off_pq), (const uint32_t*)p, L.T, i_from, i_to, merge64, d_nn_idx, d_hd_idx, d_nn_d2, d_hd_d2,
                   blocks, chunks, wpb, nn32_smem(wpb, tq, n_cols)};
  sweep_timer_mark(1, true, stream);
  switch (steps) {
#define X_(SV) case SV: nn32_sweep<SV>(A, stream); break;
    DC_FP32_INSTANCES(X_)
#undef X_
    default: assert(!"no fp32 instance for this K-step count");
  }
  sweep_timer_mark(1, false, stream);
  if (chunks > 1)
    hipLaunchKernelGGL(nn32_unpack_kernel, dim3((i_to - i_from + 255) / 256), dim3(256), 0, stream,
                       (const unsigned long long*)merge64, n_rows, i_from, i_to, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2);
}

}  // namespace dc
