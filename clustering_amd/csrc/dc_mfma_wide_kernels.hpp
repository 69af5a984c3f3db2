// dc_mfma_wide_kernels.hpp -- matrix-core sweeps for rows of 65..256 columns (gfx950, v_mfma_f32_32x32x16_f16).
// Included by dc_mfma_wide.hip and by tests/cpp/test_wide_model.hip.
//
// The sweeps of dc_mfma_kernels.hpp keep the query fragments of a chain in VGPRs (NM x 4 registers per query tile),
// which ends at 64 columns (NM = 13).  Here NEITHER operand is resident: a workgroup of four waves owns a block of
// 4 query tiles x 4 reference tiles (128 x 128 frames), every wave 2 x 2 of them as four accumulator tiles of 16
// registers, and the K axis of both operand images streams through LDS in chunks of kWideKC MFMAs (64 K slots),
// double-buffered: while the waves run the 4 x kWideKC MFMAs of a chunk, the next chunk is already on its way from
// global memory into registers, and is stored into the other buffer behind the MFMAs.  After the last chunk of a block the
// accumulators hold acc ~ S d2 for 64 x 64 pairs per wave, and the epilogue classifies them.
//
// Operand model, slot order and band are those of dc_mfma_kernels.hpp (file header, "guard band"): two fp16 pieces per
// centred, scaled coordinate, products hi*hi, mid*hi, hi*mid, the slots laid out by the same rule (two constant slots,
// then ALL hi*hi products, then the small products), C-init = reference norm (+inf for pad rows), and the chain of a
// tile pair runs its MFMAs in slot order whatever the chunking -- the chunks only decide when an operand fragment
// reaches LDS.  So the accumulator of a pair is, bit for bit, what a resident-operand chain of nm_for(D) MFMAs would
// give, and guard_e0 / guard_kappa bound it as they stand (they are written in D, nb and ns).  The folded constant is
// c_q = |x''|^2 (the neighbour form) for BOTH sweeps: one chain serves every radius of the call, so no threshold
// can be folded, and the epilogue compares acc with per-radius windows instead of reading two bits.  With that the
// population scale (band <= 1) buys nothing, and both sweeps run under pick_scale_nn: a power of two, exact.
//     | acc - S d2 |  <=  e0 + kappa S d2,     e0 = guard_e0(S M, 0, D, g = 0, a = 15, rounded = 0), kappa = guard_kappa(D, 0)
// populations, threshold t = S fl32(r^2):   acc <  t (1 - kappa) - e0  =>  d2 <  fl32(r^2)    (inside)
//                                           acc >= t (1 + kappa) + e0  =>  d2 >= fl32(r^2)    (outside)
//                                           otherwise the pair is deferred to the exact path
// neighbours, m = the least acc a lane has met so far (its own tile included): the nearest frame j* has
//     acc* <= (S d2* + e0) + kappa S d2*  and  S d2* <= S d2_j <= (acc_j + e0) / (1 - kappa)  for every j, so
//     acc* <= cut(m) = (m + e0) (1 + kappa) / (1 - kappa) + e0
// whenever it is met: every element with acc <= cut(m) is a candidate and goes to the exact path, which merges
// (d2, index) lexicographically -- ties, duplicates included, all pass the same test.  nn_hd: the same over the
// references with fe[j] < fe[i].
// Exact path: dist2_canon_rt on the original coordinates, from a per-wave LDS queue that is drained when the next
// push might not fit (never dropped) and at the end; results go out through integer atomics (counts: atomicAdd;
// neighbours: atomicMin on (d2 bits << 32 | index), finished by wide_nn_finish_kernel).
//
// The cross form (SweepMode kAgainst, dc_hip_*_cross_wide_dev): queries Q against a reference R.  The sweep is an
// every-pair sweep without symmetry, order or pruning, so a rectangle is the same chain over two images of different
// length: the A form and the norms are built from R, the B form from Q, under ONE origin (the mean of Q and R together)
// and ONE scale (pick_scale_nn of M, the largest |x'|^2 of either set).  The band holds unchanged:
//   M bounds the norm of every row of BOTH operands, which is all guard_e0 / guard_kappa ask of the data;
//   slot order and chain are those of the self sweep, so the accumulator of a pair is the same sum of the same terms.
// What differs is bookkeeping: no diagonal, no +1 for the frame itself, no i != j exclusion, outputs strided by n_query.
//
// The radius graph (WideMode kWidePairs / kWideMinEdge, dc_hip_radius_*_wide_dev): the one-radius population sweep with a
// sink on its two decision points -- the accumulator window (acc < lo: decided inside) and the exact drain (d2 < r2).
// Preparation, images, scale, band, window, shares, unit map and counting are the population sweep's; see "the sinks
// of the radius graph" below for the i < j rule of the list and the smallest-rank rule of a Boruvka round.
// Their pruned form (dc_hip_radius_*_wide_pruned_dev) is the pruned population sweep with the same sinks:
// the kernel works in positions of the order, the contract speaks of rows.  The i < j rule and the tile-level skip are
// taken on positions (each unordered pair still has exactly one meeting with i < j), the pair written is (perm[i],
// perm[j]) -- each unordered pair once, in no order within the pair; comp and rank are read by position from arrays
// gathered into the order once per call, their values and the index of best stay component ids and ranks.
// The pruned neighbour sweep (dc_hip_nearest_neighbors_wide_pruned_dev) is the neighbour form on that order
// in three launches -- the blocks next to the query block, the blocks within the bound of its nearest neighbours, the
// blocks within the bound of its lower-free-energy neighbours that hold a lower row (dc_wide_prune.hpp) --, the later
// ones starting from the merged words of the earlier; the words are placed by position and name rows.
// Both pruned self sweeps also serve rows of 257..1024 columns (dc_hip_*_xwide_pruned_dev): the same
// instances over a longer chain, with the factor of wide_nn_start and the floors of the two rules taken for the width.
// The pruned cross population sweep (dc_hip_populations_cross_wide_pruned_dev) is the pruned population
// sweep over a rectangle: the query range and the reference each in an order of its own on ONE cell grid, a set of boxes
// each; the kernel works in positions of the two orders, the scatter behind it writes rows of the query array.
// The pruned cross neighbour sweep (dc_hip_nearest_neighbors_cross_wide_pruned_dev) joins the two: the
// three launches of 4.24 on the two orders of 4.25, the seed of a query block being the one reference block whose box
// centre is nearest to its own (wide_cross_seed_kernel).
// Both pruned cross sweeps also serve rows of 257..1024 columns (dc_hip_*_cross_xwide_pruned_dev), as the
// pruned self sweeps do: the same instances, the factor and the floors of the width.
#pragma once
#include "dc_mfma_kernels.hpp"
#include "dc_mfma_wide.hpp"

namespace dc {

namespace {

constexpr int kWideKC = 4;               // MFMAs (16 K slots each) per LDS chunk
constexpr int kWideBlockTiles = 4;       // tiles per side of a workgroup's block
constexpr uint32_t kWideBlockRows = 32 * kWideBlockTiles;
constexpr uint32_t kWideQueue = 256;     // deferred pairs a wave parks before it drains them
constexpr uint32_t kWideChunkVec = kWideKC * 2 * kWideBlockTiles * 64;   // 16-byte fragments of one chunk: 2048 = 32 KiB
static_assert(kWideChunkVec % 256 == 0 && kWideQueue >= 128, "staging shape; a push of 64 fits after a drain");
// header (1024 bytes, words as in dc_mfma_kernels.hpp: 0 max |x'|^2, 1 flag, kHdrScale..+4 the scale) and behind it
// the regions the 64-column header has no room for
constexpr uint32_t kWideHdrTiles = 40, kWideHdrMfma = 42, kWideHdrExact = 44;   // 64-bit counters of the last sweep
constexpr size_t kWideOffSums = kHdrBytes;                             // [256] double: column sums
constexpr size_t kWideOffMeans = kWideOffSums + 8 * kWideMaxCols;      // [256] float: column means
constexpr size_t kWideOffImages = kWideOffMeans + 4 * kWideMaxCols;    // 4096
// The layout is a function of the maximum width of the family a column count belongs to: up to kWideMaxCols the regions
// above, byte for byte; beyond (257..1024 columns) [1024] doubles and [1024] floats, the images at 13 312
inline size_t wide_head_cols(size_t n_cols) { return n_cols <= kWideMaxCols ? kWideMaxCols : kXWideMaxCols; }
inline size_t wide_off_means(size_t n_cols) { return kWideOffSums + 8 * wide_head_cols(n_cols); }
inline size_t wide_off_images(size_t n_cols) { return wide_off_means(n_cols) + 4 * wide_head_cols(n_cols); }
static_assert(kHdrBytes + 12 * kXWideMaxCols == 13312, "the images of the 257..1024 layout start at byte 13 312");
static_assert(4 * (kWideHdrExact + 2) <= kWideInfoBytes && kWideInfoBytes <= kHdrBytes, "counters inside the info head");
static_assert(kWideHdrTiles > kHdrShift && kWideHdrTiles > kHdrScale + 4 && kWideHdrTiles % 2 == 0, "counters clear of the shared header words, 64-bit aligned");
// the pruned population sweep: extent of columns 0 / 1 as ~key(min0), key(max0), ~key(min1), key(max1)
// (words 8..11 of the 64-column header, here clear of the counters), and what order the workspace holds: mark, rows, columns
constexpr uint32_t kWideHdrExt = 48, kWideHdrOrder = 52, kWideOrderMark = 0x57504F52u;
static_assert(kWideHdrExt >= kWideHdrExact + 2 && 4 * (kWideHdrOrder + 3) <= kWideInfoBytes, "the pruned sweep's words: behind the counters, inside the info head");
// ... and of the pruned cross sweep, words of their own: a self order never passes as a cross order, nor
// the reverse (a preparation clears the whole header).  The reference's order: mark, rows, columns; behind it the
// order of the query range: mark, rows of the range, columns; then the rows of the query array the workspace is laid out for
constexpr uint32_t kWideHdrOrderRef = 56, kWideHdrOrderQuery = 59, kWideHdrOrderLaidOut = 62;
constexpr uint32_t kWideOrderMarkRef = 0x57585052u, kWideOrderMarkQuery = 0x57585051u;
static_assert(kWideHdrOrderRef >= kWideHdrOrder + 3 && 4 * (kWideHdrOrderLaidOut + 1) <= kWideInfoBytes, "the cross order's words: behind the self order's, inside the info head");
// ... and of the neighbour blocks of a sharded run (dc_hip_neighbors_block_*_wide_dev), behind the info
// head: the verdict of the last unpack (1: the gathered blocks were packed under different layouts, nothing was unpacked)
// and the 64-bit hash of the order, formed by the pack and by the unpack; a preparation clears both with the header
constexpr uint32_t kWideHdrLayoutBad = 64, kWideHdrOrderHash = 66;
static_assert(4 * kWideHdrLayoutBad >= kWideInfoBytes && kWideHdrOrderHash % 2 == 0 && 4 * (kWideHdrOrderHash + 2) <= kHdrBytes,
              "the block words: behind the info head, the hash 64-bit aligned, inside the header");
constexpr float kWidePruneCellFrames = (float)kWideBlockRows;   // frames per cell of the order's grid: one block's worth
constexpr uint32_t kWideListCap = 1024;   // surviving reference blocks a workgroup lists per scan round (4 KiB of LDS)
static_assert(kWideListCap % 256 == 0, "a round: whole chunks of 64 boxes for each of the four waves");

// Workgroup -> (query block, reference share).  A workgroup re-reads the fragments of its query block for every
// reference block it meets, and streams the reference blocks of its share: both come out of L2 only if the workgroups
// that run side by side on an XCD need few DIFFERENT blocks.  Workgroups are dealt round-robin to the 8 XCDs by their
// linear id (dc_mfma_kernels.hpp xcd_block), so the ids are decoded such that 64 consecutive workgroups of one XCD are
// 8 query blocks x 8 shares: 8 + 8 blocks in flight per XCD (1.2 MB at 100 columns, 3.1 MB at 256, of 4 MB), each
// used by 8 workgroups, and every XCD only ever touches its own eighth of the reference image.  (With the query blocks
// along x and one share per launch row, the 64 workgroups of an XCD hold 64 different query blocks: 4.9 MB at 100 columns.)
// The shares of a launch: a power of two, at most kWideShares, and no more than leave every share kWideShareBlocks
// reference blocks -- every share of a query starts its neighbour search from nothing, and a share of one block sends
// its whole first harvest of candidates to the exact path (1 500 rows: 12 blocks, one share).  With n < 64 shares the 64
// (XCD, share slot) pairs of a group are n shares x 64 / n further query blocks, so every XCD has work at every size.
constexpr uint32_t kWideShares = 64;        // reference shares at most: share s owns the reference blocks s, s + n_shares, ...
constexpr uint32_t kWideShareBlocks = 8;    // reference blocks a share holds at least (while there are that many)
// The group: gq query blocks x gs share slots side by side on an XCD (powers of two, at most 8 each).  8 x 8 is the map
// above and what every launch passes; other shapes exist for the measurement of DESIGN.md 4.31 (deep K: do fewer blocks
// per group keep the operands in L2?).  With gs share slots per XCD a launch has 8 gs of them, which caps its shares.
struct WideGroup {
  uint32_t gq, gs;
};
constexpr WideGroup kWideGroup88{8u, 8u};
__host__ __device__ inline uint32_t wide_shares(uint32_t ref_blocks, WideGroup grp = kWideGroup88) {
  uint32_t s = 1;
  while (2u * s <= 8u * grp.gs && 2u * s * kWideShareBlocks <= ref_blocks) s *= 2u;
  return s;
}
static_assert(8u * kWideGroup88.gs == kWideShares, "the 8 x 8 group hands out kWideShares share slots");
struct WideUnit {
  uint32_t q_block, share;
};
__host__ __device__ inline WideUnit wide_unit(uint32_t id, uint32_t n_shares, WideGroup grp = kWideGroup88) {
  const uint32_t xcd = id & 7u, slot = id >> 3, g = xcd * grp.gs + ((slot / grp.gq) % grp.gs), mult = 8u * grp.gs / n_shares;
  return WideUnit{((slot / (grp.gq * grp.gs)) * grp.gq + (slot % grp.gq)) * mult + g / n_shares, g % n_shares};
}
inline uint32_t wide_grid_size(uint32_t q_blocks, uint32_t n_shares, WideGroup grp = kWideGroup88) {
  const uint32_t per_group = grp.gq * (8u * grp.gs / n_shares);   // query blocks of 8 gq gs consecutive workgroups
  return 8u * grp.gq * grp.gs * ((q_blocks + per_group - 1u) / per_group);
}

struct WideLayout {
  uint32_t T, Tp, NM;   // reference tiles, tiles padded to whole blocks, MFMAs per chain
  uint32_t Tq, Tqp;     // query tiles, padded (the self sweep: T, Tp)
  size_t off_img_a, off_img_b, off_norms, off_merge, total;
};
inline uint32_t wide_pad_tiles(uint32_t T) { return (T + kWideBlockTiles - 1) / kWideBlockTiles * kWideBlockTiles; }
// n_query rows against n_ref rows: the A form and the norms of the reference, the B form and the merge words of the queries
inline WideLayout wide_layout_against(size_t n_query, size_t n_ref, size_t n_cols) {
  WideLayout L;
  L.T = (uint32_t)((n_ref + 31) / 32);
  L.Tp = wide_pad_tiles(L.T);
  L.Tq = (uint32_t)((n_query + 31) / 32);
  L.Tqp = wide_pad_tiles(L.Tq);
  L.NM = (uint32_t)nm_for((int)n_cols);
  const size_t tile_bytes = (size_t)16 * 64 * L.NM;
  L.off_img_a = wide_off_images(n_cols);
  L.off_img_b = align256(L.off_img_a + tile_bytes * L.Tp);
  L.off_norms = align256(L.off_img_b + tile_bytes * L.Tqp);
  L.off_merge = align256(L.off_norms + sizeof(float) * 32 * (size_t)L.Tp);
  L.total = align256(L.off_merge + sizeof(unsigned long long) * 2 * n_query);
  return L;
}
inline WideLayout wide_layout(size_t n_rows, size_t n_cols) { return wide_layout_against(n_rows, n_rows, n_cols); }

// ---- the band of the wide sweeps, host and device (scaled units) ------------------------------------------------------
struct WideBand {
  float e0, kappa;
};
__host__ __device__ inline WideBand wide_band(float M_scaled, int D, const Scale& sc) {
  const GuardBand gb = guard_band(M_scaled, 0.0f, D, sc);
  return WideBand{gb.e0, gb.kappa};
}
// float roundings of the window arithmetic below: a few ulp of the largest term
constexpr float kWideRoundMargin = 6.0e-7f;
// population window of one scaled threshold: [lo, hi) is undecided
__host__ __device__ inline void wide_window(float thr, const WideBand& b, float& lo, float& hi) {
  if (!(thr <= FLT_MAX)) {   // a radius beyond every float: every finite accumulator is inside
    lo = hi = INFINITY;
    return;
  }
  const float band = thr * b.kappa + b.e0, marg = (thr + b.e0) * kWideRoundMargin;
  lo = (thr - band) - marg;
  hi = (thr + band) + marg;
}
// neighbour cut of a running minimum m (+inf: nothing met yet -> +inf)
__host__ __device__ inline float wide_cut(float m, const WideBand& b, float ratio) {
  const float c = (m + b.e0) * ratio + b.e0;
  return c + fabsf(c) * kWideRoundMargin;
}
__host__ __device__ inline float wide_cut_ratio(const WideBand& b) {
  return (1.0f + b.kappa) / (1.0f - b.kappa) * (1.0f + kWideRoundMargin);
}

// The pruned neighbour sweep: the running minimum a lane starts a later launch with, from the merged word
// of the launches before (~0: nothing found -> +inf).  The word holds the canonical float sum d2_c of the row it names;
// that row's real d2 <= d2_c / (1 - u)^(D+2) <= d2_c (1 + 1.6e-5) at D <= 256, and its accumulator is at most
// S d2 (1 + kappa) + e0 by the band: m0 is that, rounded up.  Every reference whose canonical sum is <= d2_c has an
// accumulator <= m0 <= cut(m0) as well, so all that could beat or tie the word are still raised.
// grow: the factor for (1 - u)^-(D+2).  1 + 2.0e-5 holds at D <= 256 only; at 1024 columns the term is 6.1e-5, and the
// pruned self and cross instances, which serve 257..1024 columns too, take 1 + 7.0e-5 there
// (wide_nn_grow; the constants and the select stand in dc_wide_prune.hpp, where the host tests reach them).
static_assert(kWideMaxCols == 256, "wide_nn_grow, wide_pop_floor and wide_nn_floor change at this width");
__device__ __forceinline__ float wide_nn_start(unsigned long long word, float S, const WideBand& b, float grow = kWideNnGrow) {
  if (word == ~0ull) return INFINITY;
  const float d2c = __uint_as_float((uint32_t)(word >> 32));
  const float m = ((S * d2c) * grow) * (1.0f + b.kappa) + b.e0;
  return m + fabsf(m) * kWideRoundMargin;
}

// ---- statistics, scale, images: the instances of dc_mfma.hip's passes for up to kXWideMaxCols columns -----------------
// (the partial sums meet in atomics, in an order that follows the scheduling: the float means, and with them M, the images
//  and the number of pairs in the band, may differ in the last bit from run to run of one call -- any origin near the mean
//  serves, the band covers it, the results are exact either way; only the exact-pair counter is not reproducible)
__global__ void wide_colsum_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D, double* __restrict__ sums) {
  __shared__ double part[kXWideMaxCols];
  for (uint32_t k = threadIdx.x; k < D; k += blockDim.x) part[k] = 0.0;
  __syncthreads();
  const uint32_t nthreads = gridDim.x * blockDim.x;
  const uint32_t used = (nthreads / D) * D;   // stride is a multiple of D: fixed column
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)n_rows * D;
  if (id < used) {
    double s0 = 0.0, s1 = 0.0;
    size_t e = id;
    for (; e + (size_t)used < total; e += 2 * (size_t)used) {
      const float v0 = coords[e], v1 = coords[e + used];
      if (fabsf(v0) <= FLT_MAX) s0 += (double)v0;   // non-finite entries do not poison the mean
      if (fabsf(v1) <= FLT_MAX) s1 += (double)v1;
    }
    if (e < total) {
      const float v = coords[e];
      if (fabsf(v) <= FLT_MAX) s0 += (double)v;
    }
    atomicAdd(&part[id % D], s0 + s1);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < D; k += blockDim.x) atomicAdd(&sums[k], part[k]);   // every column, whatever the block holds
}

__global__ void wide_mean_kernel(const double* __restrict__ sums, size_t n_rows, uint32_t D, float* __restrict__ means) {
  for (uint32_t k = threadIdx.x; k < D; k += blockDim.x) {
    float muf = (float)(sums[k] / (double)n_rows);
    if (!(fabsf(muf) <= FLT_MAX)) muf = 0.0f;
    means[k] = muf;
  }
}

// max |x'|^2 (word 0) and the non-finite / overflow flag (word 1); one wave per row, the columns across its lanes.
// |x'|^2 is formed from the same centred floats as wide_image_kernel forms it, so word 0 bounds every norm.
__global__ void wide_rowstats_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D,
                                     const float* __restrict__ means, uint32_t* __restrict__ hdr) {
  const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  uint32_t m_norm = 0;
  bool bad = false;
  for (uint32_t row = wave; row < n_rows; row += n_waves) {
    const float* x = coords + (size_t)row * D;
    double nrm = 0.0;
    for (uint32_t k = lane; k < D; k += 64u) {
      const float v = x[k] - means[k];
      nrm += (double)v * (double)v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nrm += __shfl_xor(nrm, off, 64);
    const float nf = (float)nrm * (1.0f + 4.0e-7f);   // (the image builder sums in column order: a few ulp apart at most)
    const bool ok = nf <= kNormLimit;
    bad = bad | !ok;
    m_norm = max(m_norm, ok ? __float_as_uint(nf) : 0u);
  }
  if (lane == 0) {
    if (bad) atomicOr(hdr + 1, 1u);
    if (m_norm > __atomic_load_n(hdr, __ATOMIC_RELAXED)) atomicMax(hdr, m_norm);
  }
}

// a NaN free energy flags the data (the comparisons of the neighbour sweep are IEEE: the direct kernel answers)
__global__ void wide_fe_flag_kernel(const float* __restrict__ fe, uint32_t n_rows, uint32_t* __restrict__ hdr) {
  bool nan = false;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += gridDim.x * blockDim.x) nan = nan | (fe[i] != fe[i]);
  if (__builtin_amdgcn_ballot_w64(nan) != 0 && (threadIdx.x & 63u) == 0) atomicOr(hdr + 1, 1u);
}

// the scale of the extent M into the header (M itself: word 0 is the caller's)
__device__ __forceinline__ void wide_write_scale(uint32_t* __restrict__ hdr, float M) {
  hdr[kHdrMused] = __float_as_uint(M);
  const ScaleExp e = pick_scale_nn(M);
  hdr[kHdrScale + 0] = __float_as_uint(e.c);
  hdr[kHdrScale + 1] = __float_as_uint(e.s2);
  hdr[kHdrScale + 2] = (uint32_t)e.g;
  hdr[kHdrScale + 3] = (uint32_t)e.a;
  hdr[kHdrScale + 4] = (uint32_t)e.rounded;
}
__global__ void wide_scale_kernel(uint32_t* __restrict__ hdr) { wide_write_scale(hdr, __uint_as_float(hdr[0])); }

// Both operand images in the slot layout of dc_mfma_kernels.hpp (slot_value): one thread writes the 16-byte fragment of
// one lane of one MFMA of one tile, reference side (A form) and query side (B form: the pieces of -2x'', and in the
// two constant slots the pieces of c_q / 2^a = |x''|^2 / 2^a, which the resident-operand kernels patch in when they
// load a query).  Rows beyond n_rows and the tiles that pad the last block: zero fragments, norm +inf.
// A cross sweep builds the A form and the norms from the reference and the B form from the queries: a form whose
// pointer is null is not written (norms goes with img_a).
__global__ void wide_image_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D, uint32_t NM, uint32_t Tp,
                                  const float* __restrict__ means, const uint32_t* __restrict__ hdr,
                                  uint4* __restrict__ img_a, uint4* __restrict__ img_b, float* __restrict__ norms) {
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = (uint32_t)(id & 63), m = (uint32_t)((id >> 6) % NM), t = (uint32_t)((id >> 6) / NM);
  if (t >= Tp) return;
  const uint32_t row = 32 * t + (lane & 31), h = lane >> 5;
  const bool live = row < n_rows;
  const float* x = coords + (size_t)(live ? row : 0u) * D;
  const Scale sc = load_scale(hdr);
  auto col = [&](uint32_t k) -> float { return (x[k] - means[k]) * sc.sa; };   // x'' = 2^k fl(x - mu)
  uint32_t wa[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};
  double nrm = 0.0;
  if (live && m == 0 && h == 0)
    for (uint32_t k = 0; k < D; ++k) {
      const float v = col(k);
      nrm += (double)v * (double)v;
    }
  if (live) {
    const uint32_t s0 = 16 * m + 8 * h;
    uint32_t G = 0, k = 0;
    if (s0 >= (uint32_t)kConstSlots) {
      G = (s0 - kConstSlots) / D;
      k = (s0 - kConstSlots) - G * D;
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      uint32_t va = 0u, vb = 0u;
      if (s0 + j < (uint32_t)kConstSlots) {
        const Pieces pn = split2((float)nrm * sc.cinv);   // (as load_query splits c_q)
        va = const_a_bits(sc.a);
        vb = (j == 0) ? pn.hi : pn.mid;
      } else {
        if (G < (uint32_t)kPieceGroups) {
          const float v = col(k);
          const Pieces pa = split2(v, sc.up, sc.dn), pb = split2(-2.0f * v, sc.up, sc.dn);
          va = (G == 0u) ? pa.hi : (G == 1u ? pa.mid : pa.hi_dn);
          vb = (G == 0u) ? pb.hi : (G == 2u ? pb.mid : pb.hi_dn);
        }
        if (++k == D) {
          k = 0;
          ++G;
        }
      }
      wa[j >> 1] |= (va & 0xFFFFu) << (16 * (j & 1));
      wb[j >> 1] |= (vb & 0xFFFFu) << (16 * (j & 1));
    }
  }
  const size_t o = ((size_t)t * NM + m) * 64 + lane;
  if (img_a) img_a[o] = make_uint4(wa[0], wa[1], wa[2], wa[3]);
  if (img_b) img_b[o] = make_uint4(wb[0], wb[1], wb[2], wb[3]);
  if (img_a && m == 0 && h == 0) norms[row] = live ? (float)nrm : INFINITY;
}

inline size_t min_sz(size_t a, size_t b) { return a < b ? a : b; }
// the preparation of a call: header reset, statistics, scale, both images (dc_mfma_wide.hip wide_prepare; the model test
// runs the same launches)
// ... its first half: header reset, statistics, scale
inline int wide_stats_launches(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, void* d_ws,
                               hipStream_t s) {
  char* p = (char*)d_ws;
  uint32_t* hdr = (uint32_t*)p;
  double* sums = (double*)(p + kWideOffSums);
  float* means = (float*)(p + wide_off_means(n_cols));
  // header, counters of the last sweep, column sums
  if (hipMemsetAsync(d_ws, 0, wide_off_images(n_cols), s) != hipSuccess) return -1;
  const size_t elems = (size_t)n_rows * n_cols;
  const uint32_t sum_blocks = (uint32_t)min_sz(1024, (elems + 255) / 256);
  hipLaunchKernelGGL(wide_colsum_kernel, dim3(sum_blocks), dim3(256), 0, s, d_coords, n_rows, n_cols, sums);
  hipLaunchKernelGGL(wide_mean_kernel, dim3(1), dim3(256), 0, s, (const double*)sums, (size_t)n_rows, n_cols, means);
  const uint32_t stat_blocks = (uint32_t)min_sz(4096, ((size_t)n_rows + 3) / 4);
  hipLaunchKernelGGL(wide_rowstats_kernel, dim3(stat_blocks), dim3(256), 0, s, d_coords, n_rows, n_cols, (const float*)means, hdr);
  if (d_fe)
    hipLaunchKernelGGL(wide_fe_flag_kernel, dim3((uint32_t)min_sz(1024, ((size_t)n_rows + 255) / 256)), dim3(256), 0, s, d_fe, n_rows, hdr);
  hipLaunchKernelGGL(wide_scale_kernel, dim3(1), dim3(1), 0, s, hdr);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// ... and its second: both images and the norms of the rows of d_coords (the pruned sweep: the rows gathered into its order)
inline int wide_image_launches(const float* d_coords, uint32_t n_rows, uint32_t n_cols, void* d_ws, hipStream_t s) {
  const WideLayout L = wide_layout(n_rows, n_cols);
  char* p = (char*)d_ws;
  const size_t frags = (size_t)L.Tp * L.NM * 64;
  hipLaunchKernelGGL(wide_image_kernel, dim3((uint32_t)((frags + 255) / 256)), dim3(256), 0, s, d_coords, n_rows, n_cols, L.NM,
                     L.Tp, (const float*)(p + wide_off_means(n_cols)), (const uint32_t*)p, (uint4*)(p + L.off_img_a),
                     (uint4*)(p + L.off_img_b), (float*)(p + L.off_norms));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
inline int wide_prepare_launches(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, void* d_ws,
                                 hipStream_t s) {
  if (wide_stats_launches(d_coords, n_rows, n_cols, d_fe, d_ws, s) != 0) return -1;
  return wide_image_launches(d_coords, n_rows, n_cols, d_ws, s);
}

// ---- the order of the pruned population sweep ----------------------------------------------------------
// exact extent of columns 0 / 1 over their finite entries (header words kWideHdrExt.., zero before)
__global__ __launch_bounds__(256) void wide_extent_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D,
                                                          uint32_t* __restrict__ hdr) {
  uint32_t m[4] = {0u, 0u, 0u, 0u};
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_rows; i += gridDim.x * 256u) {
    const float x = coords[(size_t)i * D], y = coords[(size_t)i * D + 1];
    if (fabsf(x) <= FLT_MAX) {
      m[0] = max(m[0], ~fkey(x));
      m[1] = max(m[1], fkey(x));
    }
    if (fabsf(y) <= FLT_MAX) {
      m[2] = max(m[2], ~fkey(y));
      m[3] = max(m[3], fkey(y));
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m[q] = max(m[q], (uint32_t)__shfl_xor((int)m[q], off, 64));
    if ((threadIdx.x & 63u) == 0 && m[q] > __atomic_load_n(hdr + kWideHdrExt + q, __ATOMIC_RELAXED)) atomicMax(hdr + kWideHdrExt + q, m[q]);
  }
}
// The cell grid on columns 0 / 1 over that extent, as against_grid (dc_prep.hpp) lays it: the edge gives about
// kWidePruneCellFrames of the frames per cell of the bounding box, at most 4001 cells per dimension.
struct WidePruneGrid {
  float lo0, lo1, cell;
  uint32_t ny;
};
__device__ __forceinline__ WidePruneGrid wide_prune_grid(const uint32_t* __restrict__ hdr, uint32_t n_rows) {
  const uint32_t* ext = hdr + kWideHdrExt;
  WidePruneGrid g;
  g.lo0 = fkey_inv(~ext[0]);
  g.lo1 = fkey_inv(~ext[2]);
  float e0 = fkey_inv(ext[1]) - g.lo0, e1 = fkey_inv(ext[3]) - g.lo1;
  if (!(fabsf(g.lo0) <= FLT_MAX)) g.lo0 = 0.0f;
  if (!(fabsf(g.lo1) <= FLT_MAX)) g.lo1 = 0.0f;
  if (!(e0 >= 0.0f) || !(e0 <= FLT_MAX)) e0 = 0.0f;
  if (!(e1 >= 0.0f) || !(e1 <= FLT_MAX)) e1 = 0.0f;
  g.cell = fmaxf(auto_cell_of(fkey_inv(ext[1]) - fkey_inv(~ext[0]), fkey_inv(ext[3]) - fkey_inv(~ext[2]), n_rows, kWidePruneCellFrames),
                 fmaxf(e0, e1) / 4000.0f);
  if (!(g.cell > 0.0f) || !(g.cell <= FLT_MAX)) g.cell = 1.0f;   // (every row on one point of the plane: one cell)
  g.ny = (uint32_t)fminf(e1 / g.cell, 4000.0f) + 1u;
  return g;
}
// the cell key of a row from its columns 0 / 1, clamped to the grid: a row outside the extent gets an edge cell
__device__ __forceinline__ uint32_t wide_prune_key(const WidePruneGrid& g, float x, float y) {
  uint32_t key = 0;
  if (fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX) {
    const uint32_t bx = (uint32_t)fminf(fmaxf((x - g.lo0) / g.cell, 0.0f), 4000.0f);
    const uint32_t by = min((uint32_t)fminf(fmaxf((y - g.lo1) / g.cell, 0.0f), 4000.0f), g.ny - 1u);
    key = bx * g.ny + ((bx & 1u) ? g.ny - 1u - by : by);
  }
  return key;
}
// cell key and value of every row (against_key_kernel's arithmetic: the cells numbered column by column, every other
// column downwards, key 0 for a non-finite row).  n_grid: the rows the cell edge is sized for (a self sweep: n_rows; the
// cross sweep: the reference's, for both sets); row0: the number of coords' first row (the value of row i is row0 + i)
__global__ __launch_bounds__(256) void wide_prune_key_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D,
                                                             const uint32_t* __restrict__ hdr, uint32_t* __restrict__ keys,
                                                             uint32_t* __restrict__ vals, uint32_t n_grid, uint32_t row0) {
  const WidePruneGrid g = wide_prune_grid(hdr, n_grid);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_rows; i += gridDim.x * 256u) {
    keys[i] = wide_prune_key(g, coords[(size_t)i * D], coords[(size_t)i * D + 1]);
    vals[i] = row0 + i;
  }
}
// The rows gathered into the order (coords_o: [n_rows][D]) and the box of every block of kWideBlockRows positions in the
// (col 0, col 1) plane, from the original floats of its live rows; a workgroup takes two blocks.  Thread 0 signs the order
// in the three header words at `sign`: mark, rows, columns.  (n_rows: the positions; perm may name rows of a longer array.)
__global__ __launch_bounds__(256) void wide_prune_rows_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D,
                                                              const uint32_t* __restrict__ perm, uint32_t n_blocks,
                                                              float* __restrict__ coords_o, float4* __restrict__ boxes,
                                                              uint32_t* __restrict__ sign, uint32_t mark) {
  static_assert(kWideBlockRows == 128, "two waves per block of the order");
  __shared__ uint32_t s_frame[256];
  __shared__ float4 part[4];
  const uint32_t pos0 = blockIdx.x * 256u, pos = pos0 + threadIdx.x;
  const uint32_t frame = (pos < n_rows) ? perm[pos] : kInvalidFrame;
  s_frame[threadIdx.x] = frame;
  __syncthreads();
  const uint32_t rows_here = min(256u, n_rows - pos0);
  const size_t base = (size_t)pos0 * D;
#pragma unroll 4
  for (uint32_t e = threadIdx.x; e < rows_here * D; e += 256u) {
    const uint32_t r = e / D, k = e - r * D;
    coords_o[base + e] = coords[(size_t)s_frame[r] * D + k];
  }
  const bool live = frame != kInvalidFrame;
  const float x = live ? coords[(size_t)frame * D] : 0.0f, y = live ? coords[(size_t)frame * D + 1] : 0.0f;
  float lo0 = live ? x : INFINITY, hi0 = live ? x : -INFINITY;
  float lo1 = live ? y : INFINITY, hi1 = live ? y : -INFINITY;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo0 = fminf(lo0, __shfl_xor(lo0, off, 64));
    hi0 = fmaxf(hi0, __shfl_xor(hi0, off, 64));
    lo1 = fminf(lo1, __shfl_xor(lo1, off, 64));
    hi1 = fmaxf(hi1, __shfl_xor(hi1, off, 64));
  }
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = make_float4(lo0, hi0, lo1, hi1);
  __syncthreads();
  if (threadIdx.x < 2u && 2u * blockIdx.x + threadIdx.x < n_blocks) {
    const float4 a = part[2 * threadIdx.x], b = part[2 * threadIdx.x + 1];   // empty block: (+inf, -inf, ..)
    boxes[2u * blockIdx.x + threadIdx.x] = make_float4(fminf(a.x, b.x), fmaxf(a.y, b.y), fminf(a.z, b.z), fmaxf(a.w, b.w));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sign[0] = mark;
    sign[1] = n_rows;
    sign[2] = D;
  }
}
// counts by position -> populations by row: pops[k][perm[p]] = cnt[k][p]; stands down with the sweep.  pop_stride: the rows
// of a radius in pops (a self sweep: n_rows; the cross sweep: the whole query array, of which the positions are a range)
__global__ __launch_bounds__(256) void wide_prune_scatter_kernel(const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ perm,
                                                                 const uint32_t* __restrict__ cnt, uint32_t n_rows, int n_rad,
                                                                 uint32_t* __restrict__ pops, uint32_t pop_stride) {
  if (hdr[1] != 0) return;
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_rows) return;
  const uint32_t i = perm[p];
  for (int k = 0; k < n_rad; ++k) pops[(size_t)k * pop_stride + i] = cnt[(size_t)k * n_rows + p];
}
// the pruned min-edge round: component and rank of every row, by position (the values stay component ids and ranks)
__global__ __launch_bounds__(256) void wide_prune_gather_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ comp,
                                                                const uint32_t* __restrict__ rank, uint32_t n_rows,
                                                                uint32_t* __restrict__ comp_o, uint32_t* __restrict__ rank_o) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_rows) return;
  const uint32_t i = perm[p];
  comp_o[p] = comp[i];
  rank_o[p] = rank[i];
}

// the pruned neighbour sweep: the free energies by position, and per block of the order the least and the
// largest of its live rows ((+inf, -inf) for a block without one); a workgroup of 128 threads per block
__global__ __launch_bounds__(128) void wide_nn_gather_kernel(const uint32_t* __restrict__ perm, const float* __restrict__ fe,
                                                             uint32_t n_rows, float* __restrict__ fe_o, float2* __restrict__ fe_range) {
  static_assert(kWideBlockRows == 128, "two waves per block of the order");
  __shared__ float2 part[2];
  const uint32_t p = blockIdx.x * kWideBlockRows + threadIdx.x;
  const bool live = p < n_rows;
  const float f = live ? fe[perm[p]] : 0.0f;
  if (live) fe_o[p] = f;
  float lo = live ? f : INFINITY, hi = live ? f : -INFINITY;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = make_float2(lo, hi);
  __syncthreads();
  if (threadIdx.x == 0) fe_range[blockIdx.x] = make_float2(fminf(part[0].x, part[1].x), fmaxf(part[0].y, part[1].y));
}
// ... between its launches: far2[qb] = wide_nn_far2(B, floor), B the largest d2 in the words of the block's live positions,
// +inf if one of them holds none (half: 0 the nn words, 1 the hd words; floor: wide_nn_floor of the width); one thread
// per position, one result per block
__global__ __launch_bounds__(128) void wide_nn_bounds_kernel(const unsigned long long* __restrict__ merge, uint32_t n_rows,
                                                             uint32_t half, float* __restrict__ far2, float floor) {
  __shared__ float part[2];
  const uint32_t p = blockIdx.x * kWideBlockRows + threadIdx.x;
  float b = 0.0f;   // (d2 >= 0; a dead position does not raise the bound)
  if (p < n_rows) {
    const unsigned long long w = merge[(size_t)half * n_rows + p];
    b = (w == ~0ull) ? INFINITY : __uint_as_float((uint32_t)(w >> 32));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) b = fmaxf(b, __shfl_xor(b, off, 64));
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0) far2[blockIdx.x] = wide_nn_far2(fmaxf(part[0], part[1]), floor);
}
// ... and behind them: the words of position p to row perm[p] ("none", the caller's preset, stays where nothing was found
// and on the rows of other segments); stands down with the sweep
__global__ __launch_bounds__(256) void wide_nn_finish_pruned_kernel(const uint32_t* __restrict__ hdr, const unsigned long long* __restrict__ merge,
                                                                    const uint32_t* __restrict__ perm, uint32_t n_rows,
                                                                    uint32_t* __restrict__ nn_idx, float* __restrict__ nn_d2,
                                                                    uint32_t* __restrict__ hd_idx, float* __restrict__ hd_d2) {
  if (hdr[1] != 0) return;
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_rows) return;
  const unsigned long long a = merge[p], b = merge[(size_t)n_rows + p];
  const uint32_t j = perm[p];
  if (a != ~0ull) {
    nn_idx[j] = (uint32_t)a;
    nn_d2[j] = __uint_as_float((uint32_t)(a >> 32));
  }
  if (b != ~0ull) {
    hd_idx[j] = (uint32_t)b;
    hd_d2[j] = __uint_as_float((uint32_t)(b >> 32));
  }
}

// the pruned cross neighbour sweep: the free energies of ONE side by position, and per block of its
// order ONE end of their range over its live rows -- the least (the reference: want_max = 0; +inf for a block without a
// live row) or the largest (the query range: want_max = 1; -inf), as wide_nn_gather_kernel writes them side by side.  A NaN
// among them raises *flag (the cross calls: header word 1, as wide_fe_flag_kernel does; the resident reference: a word
// per side): ring 2 rests on these ends.
// Not gated on header word 1 itself: it reads through perm, which the preparation completes whatever the data holds.
__global__ __launch_bounds__(128) void wide_cross_nn_gather_kernel(const uint32_t* __restrict__ perm, const float* __restrict__ fe,
                                                                   uint32_t n_rows, uint32_t want_max, float* __restrict__ fe_o,
                                                                   float* __restrict__ fe_end, uint32_t* __restrict__ flag) {
  static_assert(kWideBlockRows == 128, "two waves per block of the order");
  __shared__ float part[2];
  const uint32_t p = blockIdx.x * kWideBlockRows + threadIdx.x;
  const bool live = p < n_rows;
  const float f = live ? fe[perm[p]] : 0.0f;
  if (live) fe_o[p] = f;
  if (__builtin_amdgcn_ballot_w64(f != f) != 0 && (threadIdx.x & 63u) == 0) atomicOr(flag, 1u);
  float v = live ? f : (want_max ? -INFINITY : INFINITY);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    v = want_max ? fmaxf(v, o) : fminf(v, o);
  }
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) fe_end[blockIdx.x] = want_max ? fmaxf(part[0], part[1]) : fminf(part[0], part[1]);
}
// ... and the seed of every query block (dc_wide_prune.hpp wide_cross_seed_key): one wave per query block, the least key
// over the reference's boxes.  n_ref_blocks >= 1, so the seed is always a block of the reference.  Not gated on header
// word 1 either: the preparation writes every box of both orders whatever the data holds (a non-finite row has key 0).
__global__ __launch_bounds__(64) void wide_cross_seed_kernel(const float4* __restrict__ qboxes, const float4* __restrict__ boxes,
                                                             uint32_t n_ref_blocks, uint32_t* __restrict__ seed) {
  const float4 q = qboxes[blockIdx.x];
  const WideBox qbox{q.x, q.y, q.z, q.w};
  unsigned long long best = ~0ull;
  for (uint32_t rb = threadIdx.x; rb < n_ref_blocks; rb += 64u) {
    const float4 b = boxes[rb];
    const unsigned long long key = wide_cross_seed_key(qbox, WideBox{b.x, b.y, b.z, b.w}, rb);
    best = key < best ? key : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o < best ? o : best;
  }
  if (threadIdx.x == 0) seed[blockIdx.x] = (uint32_t)best;
}

// ... of a cross sweep: ONE origin and ONE scale over the queries and the reference together (column sums over both
// sets, the mean over n_query + n_ref rows, header word 0 = the largest |x'|^2 of either set), then the A form and the
// norms of the reference and the B form of the queries.  d_query == d_ref is an ordinary pair of sets.
// ... its first half: header reset, statistics, scale
inline int wide_stats_against_launches(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref,
                                       uint32_t n_cols, void* d_ws, hipStream_t s) {
  char* p = (char*)d_ws;
  uint32_t* hdr = (uint32_t*)p;
  double* sums = (double*)(p + kWideOffSums);
  float* means = (float*)(p + wide_off_means(n_cols));
  if (hipMemsetAsync(d_ws, 0, wide_off_images(n_cols), s) != hipSuccess) return -1;
  struct Side {
    const float* x;
    uint32_t n;
  } const sides[2] = {{d_query, n_query}, {d_ref, n_ref}};
  for (const Side& side : sides) {
    const size_t elems = (size_t)side.n * n_cols;
    hipLaunchKernelGGL(wide_colsum_kernel, dim3((uint32_t)min_sz(1024, (elems + 255) / 256)), dim3(256), 0, s, side.x, side.n,
                       n_cols, sums);
  }
  hipLaunchKernelGGL(wide_mean_kernel, dim3(1), dim3(256), 0, s, (const double*)sums, (size_t)n_query + n_ref, n_cols, means);
  for (const Side& side : sides)
    hipLaunchKernelGGL(wide_rowstats_kernel, dim3((uint32_t)min_sz(4096, ((size_t)side.n + 3) / 4)), dim3(256), 0, s, side.x,
                       side.n, n_cols, (const float*)means, hdr);
  hipLaunchKernelGGL(wide_scale_kernel, dim3(1), dim3(1), 0, s, hdr);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// ... and its second, in a workspace laid out by L: the A form and the norms of the n_ref rows of d_ref, the B form of the
// n_query rows of d_query (the pruned cross sweep: both gathered into their orders, the queries a range of the array L is for)
inline int wide_image_against_launches(const WideLayout& L, const float* d_query, uint32_t n_query, const float* d_ref,
                                       uint32_t n_ref, uint32_t n_cols, void* d_ws, hipStream_t s) {
  char* p = (char*)d_ws;
  const float* means = (const float*)(p + wide_off_means(n_cols));
  const uint32_t Tqp = wide_pad_tiles((n_query + 31u) / 32u);
  const size_t frags_r = (size_t)L.Tp * L.NM * 64, frags_q = (size_t)Tqp * L.NM * 64;
  hipLaunchKernelGGL(wide_image_kernel, dim3((uint32_t)((frags_r + 255) / 256)), dim3(256), 0, s, d_ref, n_ref, n_cols, L.NM,
                     L.Tp, means, (const uint32_t*)p, (uint4*)(p + L.off_img_a), (uint4*)nullptr, (float*)(p + L.off_norms));
  hipLaunchKernelGGL(wide_image_kernel, dim3((uint32_t)((frags_q + 255) / 256)), dim3(256), 0, s, d_query, n_query, n_cols, L.NM,
                     Tqp, means, (const uint32_t*)p, (uint4*)nullptr, (uint4*)(p + L.off_img_b), (float*)nullptr);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
inline int wide_prepare_against_launches(const float* d_query, uint32_t n_query, const float* d_ref, uint32_t n_ref,
                                         uint32_t n_cols, void* d_ws, hipStream_t s) {
  if (wide_stats_against_launches(d_query, n_query, d_ref, n_ref, n_cols, d_ws, s) != 0) return -1;
  return wide_image_against_launches(wide_layout_against(n_query, n_ref, n_cols), d_query, n_query, d_ref, n_ref, n_cols, d_ws, s);
}

// ---- the resident reference of the pruned cross sweeps (dc_hip_reference_wide_*) -----------------------
// The reference is prepared once: origin = ITS column means, extent of columns 0 / 1 = ITS extent, and the scale that of
//   M_res = 4 M_ref,   M_ref = the largest |x - mean|^2 of the reference as wide_rowstats_kernel forms it,
// in header word 0 and kHdrMused, where M stands: a query up to twice as far from the origin as the farthest reference
// frame is inside.  The band holds as it stands: it asks only that M bounds the norm of every row of BOTH operands, which
// the reference meets with room (M_ref <= M_res) and every batch that passes wide_res_gate_kernel by that kernel's test.
// The factor is a power of two: the exponent of pick_scale_nn moves by exactly one, the scale stays a power of two.
// Header words of the resident form (behind the block words; a preparation of another form clears them with the header):
// the flags are kept apart, and word 1 -- the word every gate reads -- is formed from them in front of every sweep.
constexpr uint32_t kWideHdrResFlagRef = 72;       // the reference holds a non-finite / overflow-prone row, or 4 M_ref is beyond kNormLimit
constexpr uint32_t kWideHdrResFlagFeRef = 73;     // a NaN among the reference's free energies
constexpr uint32_t kWideHdrResFlagBatch = 74;     // the staged batch holds a row that is non-finite or beyond M_res
constexpr uint32_t kWideHdrResFlagFeQuery = 75;   // a NaN among the free energies of the last neighbour sweep's queries
constexpr uint32_t kWideHdrResAnswered = 76;      // who answered the last sweep: 0 the matrix cores, 1..3 the direct kernels (dc_density.h)
constexpr uint32_t kWideHdrResMref = 77;          // M_ref (float bits)
static_assert(kWideHdrResFlagRef >= kWideHdrOrderHash + 2 && 4 * (kWideHdrResMref + 1) <= kHdrBytes, "the resident words: behind the block words, inside the header");

// behind the reference's statistics (word 0 = M_ref, word 1 = its flag): M_res and its scale; the flag moves to its own word
__global__ void wide_res_scale_kernel(uint32_t* __restrict__ hdr) {
  const float M_ref = __uint_as_float(hdr[0]), M_res = 4.0f * M_ref;
  const bool flagged = hdr[1] != 0u || !(M_res <= kNormLimit);
  hdr[kWideHdrResMref] = __float_as_uint(M_ref);
  hdr[kWideHdrResFlagRef] = flagged ? 1u : 0u;
  const float M = (M_res <= kNormLimit) ? M_res : M_ref;   // (a flagged reference is never swept: any finite scale serves)
  hdr[0] = __float_as_uint(M);
  hdr[1] = flagged ? 1u : 0u;
  wide_write_scale(hdr, M);
}

// in front of a batch: what belongs to the batch before -- the counters, the signature of the query order, its two flags,
// who answered -- is cleared; the means, M_res, the scale, the extent and the reference's order stay
__global__ void wide_res_batch_reset_kernel(uint32_t* __restrict__ hdr) {
  const uint32_t t = threadIdx.x;
  if (t < 6u) hdr[kWideHdrTiles + t] = 0u;
  if (t < 3u) hdr[kWideHdrOrderQuery + t] = 0u;
  if (t == 0u) {
    hdr[kWideHdrResFlagBatch] = 0u;
    hdr[kWideHdrResFlagFeQuery] = 0u;
    hdr[kWideHdrResAnswered] = 0u;
    hdr[1] = hdr[kWideHdrResFlagRef];
  }
}

// The gate of a batch, its ONE pass over the rows: a wave per row, the columns across its lanes (the resident means in
// registers, SLOTS per lane: 4 for rows of 65..256 columns, 16 for 257..1024).  |x - mean|^2 as
// wide_rowstats_kernel forms it against the resident means; the batch's flag
// is raised by a row that is non-finite, beyond kNormLimit or beyond M_res (header word 0).  Columns 0 / 1 of the row are
// in lanes 0 / 1: lane 0 writes the row's cell key on the reference's grid (clamped) and its value for the sort.
// Stands in for a column-sum pass, a statistics pass, an extent pass and a key pass over the batch.  No LDS.
constexpr uint32_t kWideGateSlots = 4, kXWideGateSlots = 16;
template <uint32_t SLOTS>
__global__ __launch_bounds__(256) void wide_res_gate_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D,
                                                            const float* __restrict__ means, uint32_t* __restrict__ hdr,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                            uint32_t n_grid) {
  static_assert(kWideMaxCols <= kWideGateSlots * 64 && kXWideMaxCols <= kXWideGateSlots * 64 && kWideMinCols > 64,
                "SLOTS columns per lane at most; lanes 0 / 1 hold columns 0 / 1");
  static_assert(SLOTS == kWideGateSlots || SLOTS == kXWideGateSlots, "the two instances");
  const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  const float M_res = __uint_as_float(hdr[0]);
  const WidePruneGrid g = wide_prune_grid(hdr, n_grid);
  float mu[SLOTS];
#pragma unroll
  for (uint32_t q = 0; q < SLOTS; ++q) mu[q] = (lane + 64u * q < D) ? means[lane + 64u * q] : 0.0f;
  bool bad = false;
  for (uint32_t row = wave; row < n_rows; row += n_waves) {
    const float* x = coords + (size_t)row * D;
    double nrm = 0.0;
    float first = 0.0f;
#pragma unroll
    for (uint32_t q = 0; q < SLOTS; ++q)
      if (lane + 64u * q < D) {
        const float xk = x[lane + 64u * q];
        if (q == 0u) first = xk;
        const float v = xk - mu[q];
        nrm += (double)v * (double)v;
      }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nrm += __shfl_xor(nrm, off, 64);
    const float nf = (float)nrm * (1.0f + 4.0e-7f);
    bad = bad | !(nf <= kNormLimit) | !(nf <= M_res);
    const float c0 = __shfl(first, 0, 64), c1 = __shfl(first, 1, 64);
    if (lane == 0) {
      keys[row] = wide_prune_key(g, c0, c1);
      vals[row] = row;
    }
  }
  if (lane == 0 && bad) atomicOr(hdr + kWideHdrResFlagBatch, 1u);
}

// in front of every sweep of a staged batch: word 1 from the resident flags -- the free energies' only for a neighbour
// sweep that reads them (with_fe) --, who answers, and the counters of this sweep from zero
__global__ void wide_res_arm_kernel(uint32_t* __restrict__ hdr, uint32_t with_fe) {
  const uint32_t t = threadIdx.x;
  if (t < 6u) hdr[kWideHdrTiles + t] = 0u;
  if (t == 0u) {
    const bool ref = hdr[kWideHdrResFlagRef] != 0u, batch = hdr[kWideHdrResFlagBatch] != 0u;
    const bool fe = with_fe != 0u && (hdr[kWideHdrResFlagFeRef] | hdr[kWideHdrResFlagFeQuery]) != 0u;
    hdr[1] = (ref || batch || fe) ? 1u : 0u;
    hdr[kWideHdrResAnswered] = ref ? 1u : (batch ? 2u : (fe ? 3u : 0u));
  }
}

// ---- the sweep ------------------------------------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ON: a copy of v that the compiler cannot trace back to v (no instruction is emitted).  What is computed from the copy is
// computed where it is used instead of once in front of the block loop, where it would hold a register across the whole
// sweep -- for values that cost one instruction.  OFF: v itself, and the code of the instance is what it was.
// This steers the register allocation of one compiler, it is no property of the language: after a change of the toolchain
// compare the metadata of the instances again (scratch/wide_asm_diff.py prints .vgpr_count, .vgpr_spill_count and
// .private_segment_fixed_size; DESIGN.md 4.26 has the figures to expect).
template <bool ON>
__device__ __forceinline__ uint32_t wide_fresh(uint32_t v) {
  if constexpr (ON) asm volatile("" : "+v"(v));
  return v;
}

// kWidePairs / kWideMinEdge (the radius graph): the one-radius population sweep with a sink on its two
// decision points, the accumulator window and the exact drain; they count as kWidePop does
enum WideMode { kWidePop = 0, kWideNn = 1, kWideDump = 2, kWidePairs = 3, kWideMinEdge = 4 };
constexpr bool wide_counts(int mode) { return mode == kWidePop || mode == kWidePairs || mode == kWideMinEdge; }

struct WideArgs {
  const float* coords;
  uint32_t n_rows, n_cols, NM, Tp;
  const uint4* img_a;
  const uint4* img_b;
  const float* norms;
  uint32_t* hdr;
  uint32_t i_from, i_to;
  Rad2 rad2;                   // populations: fl32(r^2) per radius, unscaled
  int n_rad;
  uint32_t* pops;              // [n_rad][n_rows], zeroed: the sweep adds
  const float* fe;             // neighbours
  unsigned long long* merge;   // [2][n_rows] (d2 bits << 32 | index), preset to ~0
  float* dump;                 // kWideDump (the model test): acc of (reference row i, query row j) at [i * 32 Tp + j]
  // the kAgainst instances only (a zero-initialised struct is the self sweep): there coords / n_rows / Tp / img_a /
  // norms / fe are the REFERENCE's, img_b is built from the queries, i_from / i_to are query rows, and pops and merge
  // are strided by n_query
  const float* q_coords;       // [n_query][n_cols]
  uint32_t n_query;
  const float* q_fe;           // nullptr: nn only (fe is not read, no candidate of the hd half is raised)
  // the graph instances only (self sweeps of one radius, rad2.v[0]; pops as for kWidePop)
  uint2* pairs;                // kWidePairs: [capacity] (i, j), i < j (the pruned form: rows, in no order within a pair)
  unsigned long long capacity;
  unsigned long long* count;   // zeroed: the sweep adds every pair it finds, written or not
  const uint32_t* comp;        // kWideMinEdge: [n_rows] component ids
  const uint32_t* rank;        // [n_rows], a permutation
  unsigned long long* best;    // [n_rows] preset to ~0: atomicMin of (max rank << 32 | min rank)
};

// the pruned form (self population sweeps): coords / images / norms are the rows GATHERED into the spatial
// order, so the kernel sees an ordinary self problem in positions; pops counts by position
struct WidePrunedArgs : WideArgs {
  const float4* boxes;    // [blocks]: the box of every block of kWideBlockRows positions in the (col 0, col 1) plane
  uint32_t seg, n_seg;    // the query blocks seg, seg + n_seg, ... (the whole sweep: 0, 1)
  float far2;             // wide_prune_far2 of the launch's largest fl32(r^2)
  // the graph instances: comp / rank are GATHERED into the order as well (their values stay component
  // ids and ranks, best stays indexed by component id); the pair list speaks of rows
  const uint32_t* perm;   // kWidePairs, kWideNn: [n_rows] position -> row
};
// the pruned neighbour instance: fe is GATHERED into the order, merge is indexed by the query's position
// and names the reference's ROW; one launch per ring (dc_wide_prune.hpp), the bounds of a query block from the launches
// before.  A struct of its own: the argument block of the other pruned instances stays what it was.
struct WideNnPrunedArgs : WidePrunedArgs {
  uint32_t ring;             // kWideRingSeed, kWideRing1, kWideRing2
  const float* far2_nn;      // [blocks], read by rings 1 and 2
  const float* far2_hd;      // [blocks], read by ring 2
  const float2* fe_range;    // [blocks]: (least, largest) free energy of the block's live rows
};
// the pruned cross population instances: coords / img_a / norms / boxes are the REFERENCE gathered into its
// order, q_coords / img_b the query range gathered into its own, n_query the rows of that range, i_from / i_to = 0 / n_query;
// pops counts by query position.  A struct of its own, for the same reason.
struct WideCrossPrunedArgs : WidePrunedArgs {
  const float4* qboxes;      // [query blocks]: the box of every block of kWideBlockRows positions of the query order
};
// the pruned cross neighbour instance: the operands of the pruned cross population instances (q_coords and
// q_fe the query range GATHERED into its order, coords and fe the reference gathered into its own), the rings of the pruned
// neighbour instance.  far2_nn / far2_hd are per QUERY block; fe_range is not read: the two ends it holds lie in two arrays,
// the least per reference block and the largest per query block.  merge is indexed by the query's position, its hd half
// n_query behind the nn half, and names the reference's ROW.  A struct of its own, for the same reason.
struct WideCrossNnPrunedArgs : WideNnPrunedArgs {
  const float4* qboxes;      // [query blocks]
  const float* fe_min_r;     // [reference blocks], read by ring 2
  const float* fe_max_q;     // [query blocks], read by ring 2
  const uint32_t* seed;      // [query blocks]: the reference block of the seed launch
};
template <bool PR, bool NN = false, bool CROSS = false>
using WideKernelArgs = std::conditional_t<PR, std::conditional_t<NN, std::conditional_t<CROSS, WideCrossNnPrunedArgs, WideNnPrunedArgs>, std::conditional_t<CROSS, WideCrossPrunedArgs, WidePrunedArgs>>, WideArgs>;

// the deferred pairs of a wave, evaluated in the canonical order from the original coordinates, a pair per lane
template <int MODE>
__device__ __attribute__((noinline)) void wide_drain(const uint2* queue, uint32_t fill, const float* coords, uint32_t n_rows,
                                                     uint32_t n_cols, uint32_t qrow0, Rad2 rad2, void* out,
                                                     const float* q_coords) {
  // (n_rows: the QUERY rows, the stride of the output; i indexes coords, the reference side; q_coords: the query rows,
  //  coords itself in the self sweep.  out: the populations or the merge words, by MODE.  The order of the parameters
  //  matters to the code: with a second pointer in FRONT of rad2 the compiler passes rad2 through scratch, a store of
  //  eight dwords at each of the 65 call sites of a population instance -- check .private_segment_fixed_size after a change)
  uint32_t* const pops = static_cast<uint32_t*>(out);
  unsigned long long* const merge = static_cast<unsigned long long*>(out);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the queue writes of all lanes before their reads)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t e = lane; e < fill; e += 64u) {
    const uint2 en = queue[e];
    const uint32_t i = en.x, j = qrow0 + (en.y & 127u), flags = en.y >> 8;
    const float d2 = dist2_canon_rt(q_coords + (size_t)j * n_cols, 1, coords + (size_t)i * n_cols, 1, (int)n_cols);
    if constexpr (MODE == kWidePop) {
#pragma unroll
      for (int k = 0; k < kMaxRadiiPerLaunch; ++k)
        if (((flags >> k) & 1u) && d2 < rad2.v[k]) atomicAdd(&pops[(size_t)k * n_rows + j], 1u);
    } else {
      const unsigned long long w = ((unsigned long long)__float_as_uint(d2) << 32) | i;
      if (flags & 1u) atomicMin(&merge[j], w);
      if (flags & 2u) atomicMin(&merge[(size_t)n_rows + j], w);
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// ---- the sinks of the radius graph (kWidePairs, kWideMinEdge) -----------------------------------------------------------
// kWidePairs.  The every-pair sweep meets an unordered pair {a, b} twice, as (reference a, query b) and as (reference b,
// query a), in different workgroups, shares, waves or halves of a wave.  Both meetings COUNT (each end's population needs
// the other), and exactly one EMITS: the one with reference row i < query row j.  Whether that meeting decides the pair
// in the accumulator window or in the drain does not matter: the rule is applied at both places.
// kWideMinEdge.  The weight of a pair is (max rank, min rank), compared lexicographically, and the ranks are a permutation.
// For a fixed query q of rank a, a partner of rank b has the key (a, b) if b < a and (b, a) if b > a.  Every b < a gives
// the high word a, every b > a a larger high word, so all partners below a come before all partners above a; among
// those below, the low word b orders them; among those above, the high word b does.  Hence over ANY set of partners the
// lightest key is the key of the partner of SMALLEST rank, and a lane carries one 32-bit running minimum of ranks per
// query tile instead of a 64-bit key.  A query's partners are split over shares, the two waves of a query tile, the two
// halves of a wave and the drain: each part's smallest rank gives that part's lightest key, and the 64-bit atomicMin on
// best[comp[q]] merges the parts -- and the queries of a component -- into the definition's minimum.

// n slots of the pair list for the wave: ONE atomic, by lane 0, the base broadcast (every lane of the wave is active)
__device__ __forceinline__ unsigned long long wide_reserve(unsigned long long* count, uint32_t n, uint32_t lane) {
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(count, (unsigned long long)n);
  const uint32_t b_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
  const uint32_t b_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
  return ((unsigned long long)b_hi << 32) | b_lo;
}
// wide_drain for the graph instances: the deferred pairs of one threshold, counted as kWidePop counts them and handed to
// the sink.  A function of its own: one float instead of the eight of Rad2, a sink behind it -- and wide_drain's
// parameter list, which is what keeps rad2 out of scratch in the population instances, stays as it is.  Called with
// every lane of the wave active; the loop is wave-uniform (one ballot and one atomic on the count per pass).
// The sink is three scalars -- kWidePairs: the list, its capacity, the count; kWideMinEdge: comp, rank, best -- and not a
// struct: a struct of three pointers is passed through the stack, 24 bytes stored at each of the 65 call sites.
// The pruned form sweeps POSITIONS of the spatial order: coords, pops, comp and rank are by position, so
// the min-edge sink is the same code; the pair list speaks of rows, so its sink takes the permutation as a fourth scalar
// -- a pack, empty for every other instance, whose code therefore stays what it was.  The i < j rule is on positions.
__device__ __forceinline__ uint2 wide_pair_ids(uint32_t i, uint32_t j) { return make_uint2(i, j); }
__device__ __forceinline__ uint2 wide_pair_ids(uint32_t i, uint32_t j, const uint32_t* perm) { return make_uint2(perm[i], perm[j]); }
template <int MODE, class A, class B, class C, class... P>
__device__ __forceinline__ void wide_graph_drain_body(const uint2* queue, uint32_t fill, const float* coords, uint32_t n_cols,
                                                      uint32_t qrow0, float r2, uint32_t* pops, A s0, B s1, C s2, P... perm) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t e0 = 0; e0 < fill; e0 += 64u) {
    const bool valid = e0 + lane < fill;
    const uint2 en = queue[valid ? e0 + lane : 0u];
    const uint32_t i = en.x, j = qrow0 + (en.y & 127u);
    const float d2 = dist2_canon_rt(coords + (size_t)j * n_cols, 1, coords + (size_t)i * n_cols, 1, (int)n_cols);
    const bool hit = valid && d2 < r2;
    if (hit) atomicAdd(&pops[j], 1u);
    if constexpr (MODE == kWidePairs) {
      const bool emit = hit && i < j;
      const unsigned long long mk = __builtin_amdgcn_ballot_w64(emit);
      if (mk != 0) {
        const unsigned long long slot = wide_reserve(s2, (uint32_t)__popcll(mk), lane) + lanes_below(mk);
        if (emit && slot < s1) s0[slot] = wide_pair_ids(i, j, perm...);
      }
    } else {
      if (hit) {
        const uint32_t cj = s0[j];
        if (s0[i] != cj) {
          const uint32_t ri = s1[i], rj = s1[j];
          atomicMin(&s2[cj], ((unsigned long long)max(ri, rj) << 32) | min(ri, rj));
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}
template <int MODE, class A, class B, class C>
__device__ __attribute__((noinline)) void wide_graph_drain(const uint2* queue, uint32_t fill, const float* coords, uint32_t n_rows,
                                                           uint32_t n_cols, uint32_t qrow0, float r2, uint32_t* pops, A s0, B s1,
                                                           C s2) {
  wide_graph_drain_body<MODE>(queue, fill, coords, n_cols, qrow0, r2, pops, s0, s1, s2);
}
// ... of the pruned pair list: (i, j) are positions, the pair written is (perm[i], perm[j])
__device__ __attribute__((noinline)) void wide_pairs_drain_pruned(const uint2* queue, uint32_t fill, const float* coords,
                                                                  uint32_t n_cols, uint32_t qrow0, float r2, uint32_t* pops,
                                                                  uint2* pairs, unsigned long long capacity,
                                                                  unsigned long long* count, const uint32_t* perm) {
  wide_graph_drain_body<kWidePairs>(queue, fill, coords, n_cols, qrow0, r2, pops, pairs, capacity, count, perm);
}

// ... of the pruned neighbour sweep: (i, j) are positions and so is the word's place, the reference it
// names is the row perm[i] -- the contract's tie rule is the least (d2, ROW).  A function of its own for wide_drain's reason.
__device__ __attribute__((noinline)) void wide_nn_drain_pruned(const uint2* queue, uint32_t fill, const float* coords,
                                                               uint32_t n_rows, uint32_t n_cols, uint32_t qrow0,
                                                               unsigned long long* merge, const uint32_t* perm) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t e = lane; e < fill; e += 64u) {
    const uint2 en = queue[e];
    const uint32_t i = en.x, j = qrow0 + (en.y & 127u), flags = en.y >> 8;
    const float d2 = dist2_canon_rt(coords + (size_t)j * n_cols, 1, coords + (size_t)i * n_cols, 1, (int)n_cols);
    const unsigned long long w = ((unsigned long long)__float_as_uint(d2) << 32) | perm[i];
    if (flags & 1u) atomicMin(&merge[j], w);
    if (flags & 2u) atomicMin(&merge[(size_t)n_rows + j], w);
  }
  __builtin_amdgcn_wave_barrier();
}

// ... of the pruned cross neighbour sweep: i is a position of the gathered reference, j one of the gathered
// query range; the word lies at the query's position (the hd half n_query behind) and names the reference's row perm_r[i]
__device__ __attribute__((noinline)) void wide_nn_drain_cross_pruned(const uint2* queue, uint32_t fill, const float* coords,
                                                                     uint32_t n_query, uint32_t n_cols, uint32_t qrow0,
                                                                     unsigned long long* merge, const uint32_t* perm_r,
                                                                     const float* q_coords) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t e = lane; e < fill; e += 64u) {
    const uint2 en = queue[e];
    const uint32_t i = en.x, j = qrow0 + (en.y & 127u), flags = en.y >> 8;
    const float d2 = dist2_canon_rt(q_coords + (size_t)j * n_cols, 1, coords + (size_t)i * n_cols, 1, (int)n_cols);
    const unsigned long long w = ((unsigned long long)__float_as_uint(d2) << 32) | perm_r[i];
    if (flags & 1u) atomicMin(&merge[j], w);
    if (flags & 2u) atomicMin(&merge[(size_t)n_query + j], w);
  }
  __builtin_amdgcn_wave_barrier();
}

// SM: kSelf -- queries and reference are the rows of one array: the diagonal pair leaves the sweep, populations get the
// frame's own 1, a frame is not its own neighbour; kAgainst -- X.q_coords against X.coords: every pair counts.
// PR: the pruned form.  A workgroup still owns (query block, share); it first scans the boxes of its share's blocks
// y, y + Sy, ... against the box of its query block -- 64 per wave and step, a ballot each -- and compacts the survivors
// (wide_prune_survives) into an LDS list, in rounds of kWideListCap blocks; the chunk sequence then runs over the list.
// A round without a survivor runs no chunk and fetches nothing.
// The pruned neighbour instance is launched once per ring; its survivors are the blocks of that ring
// (wide_nn_ring), rings 1 and 2 start the running minima from the merged words, and the words name rows.
// The pruned cross population instances: two orders, two sets of boxes.  The query block is a block of
// the QUERY order (its count bounds it, its box comes from X.qboxes), the scanned boxes and the listed blocks are the
// reference's; rows, live[] and the drain speak of positions of the gathered query range [0, n_query) against positions
// of the gathered reference, as the unpruned cross form speaks of rows; there is no segment.
// The pruned cross neighbour instance is that form with the rings: the seed of a query block is the one
// reference block X.seed names, the bounds and the largest free energy are the QUERY block's, the least free energy the
// reference block's, the words lie by query position and name rows of the reference.
// GQ x GS: the group of the unit map (8 x 8 in every instance the library launches; see WideGroup).
template <int MODE, int NR, SweepMode SM = kSelf, bool PR = false, uint32_t GQ = 8u, uint32_t GS = 8u>
__global__ __launch_bounds__(256, 2) void wide_sweep_kernel(WideKernelArgs<PR, MODE == kWideNn, PR && SM == kAgainst> X) {
  static_assert(!PR || ((wide_counts(MODE) || MODE == kWideNn) && SM == kSelf) || (MODE == kWidePop && SM == kAgainst && (NR == 1 || NR == 4 || NR == kMaxRadiiPerLaunch)) ||
                    (MODE == kWideNn && SM == kAgainst && NR == 1),
                "the pruned form: self sweeps -- populations, the radius graph, neighbours -- and the cross population and neighbour sweeps");
  if (X.hdr[1] != 0) return;   // non-finite / overflow-prone data: the gated direct kernel runs instead
  __shared__ uint32_t list_s[PR ? kWideListCap : 1];                  // pruned: the surviving reference blocks of a round
  __shared__ unsigned long long mask_s[PR ? kWideListCap / 64 : 1];   // ... and the ballots they are compacted from
  __shared__ u32x4 stage[2 * kWideChunkVec];
  __shared__ uint2 queue_s[4][kWideQueue];
  __shared__ float fe_s[kWideBlockRows];
  __shared__ float min_s[4][2][2][32];   // neighbours: running minima (nn, nn_hd) per wave and query, exchanged per block
  __shared__ uint2 cr_s[kWideBlockRows];  // min edge: (component, rank) of the reference block's rows
  constexpr bool kCount = wide_counts(MODE);
  // the pruned cross neighbour instance has no register to spare: 256 and 14 spilled without this, 0 spilled with it
  constexpr bool kFresh = PR && MODE == kWideNn && SM == kAgainst;
  static_assert((MODE != kWidePairs && MODE != kWideMinEdge) || (NR == 1 && SM == kSelf), "the graph instances: one radius, self sweeps");
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, h = lane >> 5, c = lane & 31u;
  const uint32_t wq = wave & 1u, wr = wave >> 1;
  const uint32_t NM = X.NM, NC = (NM + kWideKC - 1) / kWideKC, D = X.n_cols;
  const float* const q_coords = (SM == kAgainst) ? X.q_coords : X.coords;
  const float* const q_fe = (SM == kAgainst) ? X.q_fe : X.fe;
  const uint32_t n_q = (SM == kAgainst) ? X.n_query : X.n_rows;
  const bool has_fe = SM == kSelf || q_fe != nullptr;
  constexpr WideGroup kGroup{GQ, GS};
  static_assert(!PR || (GQ == 8u && GS == 8u), "the pruned forms run on the 8 x 8 map");
  const uint32_t RB = X.Tp / kWideBlockTiles, Sy = wide_shares(RB, kGroup);
  const WideUnit unit = wide_unit(blockIdx.x, Sy, kGroup);
  uint32_t qb_of_unit = X.i_from / kWideBlockRows + unit.q_block;
  // (the pruned cross form: i_from = 0, so this is the unit's block of the query order, bounded below by that order's
  //  length -- the reference's block count RB says nothing about it)
  if constexpr (PR && SM == kSelf) {   // every n_seg-th block of the order (64 bits: n_seg is any number)
    const unsigned long long q = X.seg + (unsigned long long)unit.q_block * X.n_seg;
    if (q >= RB) return;
    qb_of_unit = (uint32_t)q;
  }
  const uint32_t qb = qb_of_unit, y = unit.share;
  // (whole workgroups: the query blocks that pad the last group)
  if (qb * kWideBlockRows >= X.i_to) return;
  const uint32_t nblk = (RB - y + Sy - 1) / Sy, n_it = nblk * NC;
  uint2* queue = queue_s[wave];
  uint32_t fill = 0;
  unsigned long long n_exact = 0;
  unsigned long long n_found = 0;   // kWidePairs, counting only: the pairs this wave decided inside, from their i < j meeting

  const Scale sc = load_scale(X.hdr);
  const WideBand band = wide_band(__uint_as_float(X.hdr[0]) * sc.s2, (int)D, sc);

  // per query tile of this wave: the lane's row
  uint32_t jq[2];
  bool live[2];
  unsigned long long livemask[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    jq[qt] = (qb * kWideBlockTiles + 2 * wq + qt) * 32 + c;
    live[qt] = jq[qt] >= X.i_from && jq[qt] < X.i_to;
    livemask[qt] = __builtin_amdgcn_ballot_w64(live[qt]);
  }

  // populations: windows and counts; neighbours: running minima
  float lo[NR], hi[NR], hi_max = -INFINITY;
  uint32_t cnt[2][NR];
  float m_nn[2], m_hd[2], feq[2];
  const float ratio = wide_cut_ratio(band);
  if constexpr (kCount) {
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      lo[k] = hi[k] = -INFINITY;   // (a radius the launch does not have: nothing inside, nothing undecided)
      if (k < X.n_rad) wide_window(X.rad2.v[k] * sc.s2, band, lo[k], hi[k]);
      hi_max = fmaxf(hi_max, hi[k]);
      cnt[0][k] = cnt[1][k] = 0;
    }
  }
  if constexpr (MODE == kWideNn) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      m_nn[qt] = m_hd[qt] = INFINITY;
      feq[qt] = (live[qt] && has_fe) ? q_fe[jq[qt]] : -INFINITY;   // (a dead lane, nn only: no reference lies lower)
      if constexpr (PR) {
        // rings 1 and 2 start from the words of the launches before: a bound on the accumulator of the row a word names
        // (the factor of the width, in the self and in the cross instance: a wave-uniform select on D, no register of a
        //  lane's -- the cross instance has none to spare, see kFresh)
        if (X.ring != kWideRingSeed && live[qt]) {
          const float grow = wide_nn_grow(D);
          m_nn[qt] = wide_nn_start(X.merge[jq[qt]], sc.s2, band, grow);
          m_hd[qt] = wide_nn_start(X.merge[(size_t)(SM == kAgainst ? n_q : X.n_rows) + jq[qt]], sc.s2, band, grow);
        }
      }
    }
  }
  // min edge: component and rank of the lane's queries, the smallest rank met among their partners of another component
  uint32_t comp_q[2], rank_q[2], rmin[2];
  if constexpr (MODE == kWideMinEdge) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      comp_q[qt] = live[qt] ? X.comp[jq[qt]] : 0u;
      rank_q[qt] = live[qt] ? X.rank[jq[qt]] : 0u;
      rmin[qt] = ~0u;
    }
  }

  // the pruned pair list: the rows of the lane's queries (the kernel's own indices are positions of the order)
  uint32_t row_q[2] = {0u, 0u};
  if constexpr (PR && MODE == kWidePairs) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) row_q[qt] = live[qt] ? X.perm[jq[qt]] : 0u;
  }

  // one pair per lane into the wave's queue (ok: this lane has one); drained before a push that might not fit
  auto drain = [&]() {
    if constexpr (PR && MODE == kWideNn && SM == kAgainst)
      wide_nn_drain_cross_pruned(queue, fill, X.coords, n_q, D, qb * kWideBlockRows, X.merge, X.perm, q_coords);
    else if constexpr (PR && MODE == kWideNn)
      wide_nn_drain_pruned(queue, fill, X.coords, n_q, D, qb * kWideBlockRows, X.merge, X.perm);
    else if constexpr (PR && MODE == kWidePairs)
      wide_pairs_drain_pruned(queue, fill, X.coords, D, qb * kWideBlockRows, X.rad2.v[0], X.pops, X.pairs, X.capacity, X.count,
                              X.perm);
    else if constexpr (MODE == kWidePairs)
      wide_graph_drain<MODE>(queue, fill, X.coords, n_q, D, qb * kWideBlockRows, X.rad2.v[0], X.pops,
                             X.pairs, X.capacity, X.count);
    else if constexpr (MODE == kWideMinEdge)
      wide_graph_drain<MODE>(queue, fill, X.coords, n_q, D, qb * kWideBlockRows, X.rad2.v[0], X.pops,
                             X.comp, X.rank, X.best);
    else
      wide_drain<MODE == kWideNn ? kWideNn : kWidePop>(queue, fill, X.coords, n_q, D, qb * kWideBlockRows, X.rad2,
                                                       MODE == kWideNn ? (void*)X.merge : (void*)X.pops, q_coords);
  };
  auto push = [&](bool ok, uint32_t i, uint32_t word) {
    const unsigned long long mk = __builtin_amdgcn_ballot_w64(ok);
    if (mk == 0) return;
    if (fill + 64u > kWideQueue) {
      drain();
      n_exact += fill;
      fill = 0;
    }
    if (ok) queue[fill + lanes_below(mk)] = make_uint2(i, word);
    fill += (uint32_t)__popcll(mk);
  };

  // chunk `it` of the workgroup's sequence (block it / NC, chunk it % NC) -> registers -> LDS buffer
  // (the last chunk of a chain may hold fewer than kWideKC MFMAs: the surplus slots re-load the chunk's last MFMA and are
  //  never read -- unconditional loads and stores keep `pre` in registers and the eight loads in flight together)
  // (u32x4, a native vector type: an array of HIP's uint4 -- a struct -- is kept in scratch, with a wait and a scratch store
  //  behind every load)
  // block `blk` of the workgroup's sequence: of its share, or -- pruned -- of the round's list of survivors
  auto ref_block = [&](uint32_t blk) -> uint32_t {
    if constexpr (PR)
      return (uint32_t)__builtin_amdgcn_readfirstlane((int)list_s[blk]);
    else
      return y + blk * Sy;
  };
  u32x4 pre[kWideChunkVec / 256];
  auto fetch = [&](uint32_t it) {
    const uint32_t blk = it / NC, ch = it - blk * NC, rb = ref_block(blk);
    const uint32_t m0 = ch * kWideKC, nmc = min((uint32_t)kWideKC, NM - m0);
#pragma unroll
    for (uint32_t i = 0; i < kWideChunkVec / 256; ++i) {
      const uint32_t e = tid + 256u * i, ml = min(e >> 9, nmc - 1u), tl = (e >> 6) & 7u;   // (MFMA of the chunk, tile 0..3 reference / 4..7 query)
      const uint32_t t = (tl < 4u) ? rb * kWideBlockTiles + tl : qb * kWideBlockTiles + (tl - 4u);
      const u32x4* img = reinterpret_cast<const u32x4*>((tl < 4u) ? X.img_a : X.img_b);
      pre[i] = img[((size_t)t * NM + m0 + ml) * 64 + lane];
    }
  };
  auto store = [&](uint32_t it) {
    u32x4* dst = stage + (it & 1u) * kWideChunkVec;
#pragma unroll
    for (uint32_t i = 0; i < kWideChunkVec / 256; ++i) dst[tid + 256u * i] = pre[i];
  };

  f32x16 acc[2][2];
  uint32_t n_eval = PR ? 0u : nblk;   // reference blocks this workgroup evaluates
  WideBox qbox{};
  if constexpr (PR && SM == kAgainst) {
    const float4 b = X.qboxes[qb];
    qbox = WideBox{b.x, b.y, b.z, b.w};
  } else if constexpr (PR) {
    const float4 b = X.boxes[qb];
    qbox = WideBox{b.x, b.y, b.z, b.w};
  }
  // the neighbour instance: the bounds of the query block (wave-uniform; a ring reads what the launches before it wrote)
  float far2_nn = 0.0f, far2_hd = 0.0f, fe_max_q = 0.0f;
  uint32_t seed_rb = 0u;   // the cross form: the reference block of the query block's seed launch
  if constexpr (PR && MODE == kWideNn) {
    if (X.ring >= kWideRing1) far2_nn = X.far2_nn[qb];
    if (X.ring == kWideRing2) {
      far2_hd = X.far2_hd[qb];
      if constexpr (SM == kAgainst)
        fe_max_q = X.fe_max_q[qb];
      else
        fe_max_q = X.fe_range[qb].y;
    }
    if constexpr (SM == kAgainst) seed_rb = X.seed[qb];
  }
  uint32_t round0 = 0;
  do {
    uint32_t n_run = n_it;   // chunks of this round (unpruned: one round, every block of the share)
    if constexpr (PR) {
      // ---- scan: which of the share's blocks round0 .. round0 + lim can hold a pair within the largest radius?
      const uint32_t lim = min(nblk - round0, kWideListCap), n_ck = (lim + 63u) >> 6;
      for (uint32_t ck = wave; ck < n_ck; ck += 4u) {
        const uint32_t e = ck * 64u + lane;
        bool ok = false;
        if (e < lim) {
          const uint32_t rb = y + (round0 + e) * Sy;
          const float4 b = X.boxes[rb];
          if constexpr (MODE == kWideNn && SM == kAgainst) {
            const float fe_min_r = (X.ring == kWideRing2) ? X.fe_min_r[rb] : 0.0f;
            ok = wide_nn_ring(wide_cross_is_seed(seed_rb, rb), wide_box_gap2(qbox, WideBox{b.x, b.y, b.z, b.w}), far2_nn, far2_hd,
                              fe_min_r, fe_max_q) == (int)X.ring;
          } else if constexpr (MODE == kWideNn) {
            const float fe_min_r = (X.ring == kWideRing2) ? X.fe_range[rb].x : 0.0f;
            ok = wide_nn_ring(wide_nn_is_seed(qb, rb), wide_box_gap2(qbox, WideBox{b.x, b.y, b.z, b.w}), far2_nn, far2_hd, fe_min_r,
                              fe_max_q) == (int)X.ring;
          } else {
            ok = wide_prune_survives(qbox, WideBox{b.x, b.y, b.z, b.w}, X.far2);
          }
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        if (lane == 0) mask_s[ck] = m;
      }
      __syncthreads();
      // every wave adds up all ballots (the count is uniform); the wave that took a chunk lists its survivors
      uint32_t cnt = 0;
      for (uint32_t ck = 0; ck < n_ck; ++ck) {
        const unsigned long long m = mask_s[ck];
        if ((ck & 3u) == wave && ((m >> lane) & 1ull)) list_s[cnt + lanes_below(m)] = y + (round0 + ck * 64u + lane) * Sy;
        cnt += (uint32_t)__popcll(m);
      }
      __syncthreads();   // (the list before its readers; the ballots before the next round writes them)
      n_eval += cnt;
      n_run = cnt * NC;
    }
    if (!PR || n_run != 0) {
      fetch(0);
      store(0);
      __syncthreads();
      for (uint32_t it = 0; it < n_run; ++it) {
        const uint32_t blk = it / NC, ch = it - blk * NC, rb = ref_block(blk);
        const uint32_t nmc = min((uint32_t)kWideKC, NM - ch * kWideKC);
        const bool last = ch == NC - 1;
        if (ch == 0) {
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            float4 nv[4];
            load_frag(X.norms, rb * kWideBlockTiles + 2 * wr + rt, (int)h, nv);
            acc[rt][0] = frag16(nv);
            acc[rt][1] = acc[rt][0];
          }
          if constexpr (MODE == kWideNn) {
            // (read by the epilogue of this block's LAST chunk, a barrier later; the previous block's epilogue ended before
            //  the barrier that closed its last chunk)
            if (tid < kWideBlockRows) {
              const uint32_t row = rb * kWideBlockRows + tid;
              fe_s[tid] = (row < X.n_rows && has_fe) ? X.fe[row] : INFINITY;
            }
          }
          if constexpr (MODE == kWideMinEdge) {   // (as fe_s: read a barrier later, written behind the last epilogue's barrier)
            if (tid < kWideBlockRows) {
              const uint32_t row = rb * kWideBlockRows + tid;
              cr_s[tid] = (row < X.n_rows) ? make_uint2(X.comp[row], X.rank[row]) : make_uint2(0u, ~0u);
            }
          }
        }
        // the next chunk leaves for the registers before this chunk's MFMAs (behind the norm loads above: the memory counter
        // is in order, and the wait for the norms must not wait for the chunk)
        if (it + 1 < n_run) fetch(it + 1);
        const u32x4* sb = stage + (it & 1u) * kWideChunkVec;
#pragma unroll
        for (uint32_t ml = 0; ml < (uint32_t)kWideKC; ++ml) {
          if (ml < nmc) {
            const s16x8 a0 = __builtin_bit_cast(s16x8, sb[(ml * 8 + 2 * wr) * 64 + lane]);
            const s16x8 a1 = __builtin_bit_cast(s16x8, sb[(ml * 8 + 2 * wr + 1) * 64 + lane]);
            const s16x8 b0 = __builtin_bit_cast(s16x8, sb[(ml * 8 + 4 + 2 * wq) * 64 + lane]);
            const s16x8 b1 = __builtin_bit_cast(s16x8, sb[(ml * 8 + 5 + 2 * wq) * 64 + lane]);
            acc[0][0] = mfma16(a0, b0, acc[0][0]);
            acc[0][1] = mfma16(a0, b1, acc[0][1]);
            acc[1][0] = mfma16(a1, b0, acc[1][0]);
            acc[1][1] = mfma16(a1, b1, acc[1][1]);
          }
        }
        if (last) {
          // ---- epilogue of the block: acc[rt][qt][g] ~ S d2(reference row of (rt, g, h), query jq[qt]) ----
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
              if (MODE != kWideDump && SM == kSelf && rb * kWideBlockTiles + 2 * wr + rt == qb * kWideBlockTiles + 2 * wq + qt) {
                // the diagonal tile: the self pair leaves the sweep (populations add their 1 at the end, neighbours exclude it)
#pragma unroll
                for (int g = 0; g < 16; ++g)
                  if (tile_row_local(g, (int)h) == c) acc[rt][qt][g] = INFINITY;
              }
          if constexpr (MODE == kWideDump) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
              for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                  const uint32_t i = (rb * kWideBlockTiles + 2 * wr + rt) * 32 + tile_row_local(g, (int)h);
                  X.dump[(size_t)i * (32u * X.Tp) + jq[qt]] = acc[rt][qt][g];
                }
          }
          if constexpr (kCount) {
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
              for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                  const float v = acc[rt][qt][g];
                  if (__builtin_amdgcn_ballot_w64(v < hi_max) == 0) continue;   // outside every radius, the whole wave
                  uint32_t und = 0;
#pragma unroll
                  for (int k = 0; k < NR; ++k) {
                    cnt[qt][k] += (v < lo[k]) ? 1u : 0u;
                    und |= ((v >= lo[k]) & (v < hi[k])) ? (1u << k) : 0u;
                  }
                  if ((__builtin_amdgcn_ballot_w64(und != 0) & livemask[qt]) != 0) {
                    const uint32_t i = (rb * kWideBlockTiles + 2 * wr + rt) * 32 + tile_row_local(g, (int)h);
                    push(und != 0 && live[qt] && i < X.n_rows, i, ((2 * wq + qt) * 32 + c) | (und << 8));
                  }
                }
                if constexpr (MODE == kWideMinEdge) {
                  // (the self pair is +inf on the diagonal tile and of the query's own component; a pad row is +inf)
#pragma unroll
                  for (int g = 0; g < 16; ++g) {
                    const uint2 cr = cr_s[(2 * wr + rt) * 32 + tile_row_local(g, (int)h)];
                    rmin[qt] = min(rmin[qt], (acc[rt][qt][g] < lo[0] && cr.x != comp_q[qt]) ? cr.y : ~0u);
                  }
                }
              }
            if constexpr (MODE == kWidePairs) {
              // the pairs this block decided inside, each from its meeting with i < j.  A reference tile above the query tile
              // holds no such element (wave-uniform; it has been counted above all the same).  The slots of the wave's four
              // tiles come from ONE atomic: a ballot per element, the popcounts summed on the scalar side, and a lane's slot
              // is the base + the popcounts of the earlier elements + the set lanes below it.  Every wave of the grid adds
              // to the same word, which takes an add every ~10 ns: one per tile made a dense list 6 x the population sweep.
              // Counting only (no list: capacity 0) needs no slot: the wave keeps its sum and adds it once, at the end.
              const uint32_t rt0 = rb * kWideBlockTiles + 2 * wr, qt0 = qb * kWideBlockTiles + 2 * wq;
              auto inside = [&](int rt, int qt, int g) {
                const uint32_t i = (rt0 + rt) * 32 + tile_row_local(g, (int)h);
                return acc[rt][qt][g] < lo[0] && live[qt] && i < X.n_rows && i < jq[qt];
              };
              uint32_t total = 0;
#pragma unroll
              for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
                  if (rt0 + rt <= qt0 + qt) {
#pragma unroll
                    for (int g = 0; g < 16; ++g) total += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(inside(rt, qt, g)));
                  }
              if (X.capacity == 0) {
                n_found += total;
              } else if (total != 0) {
                unsigned long long slot0 = wide_reserve(X.count, total, lane);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                  for (int rt = 0; rt < 2; ++rt)
                    if (rt0 + rt <= qt0 + qt) {
#pragma unroll
                      for (int g = 0; g < 16; ++g) {
                        const bool ok = inside(rt, qt, g);
                        const unsigned long long mk = __builtin_amdgcn_ballot_w64(ok);
                        const unsigned long long slot = slot0 + lanes_below(mk);
                        if (ok && slot < X.capacity) {
                          const uint32_t i = (rt0 + rt) * 32 + tile_row_local(g, (int)h);
                          if constexpr (PR)
                            X.pairs[slot] = make_uint2(X.perm[i], row_q[qt]);
                          else
                            X.pairs[slot] = make_uint2(i, jq[qt]);
                        }
                        slot0 += (unsigned long long)__popcll(mk);
                      }
                    }
              }
            }
          }
          if constexpr (MODE == kWideNn) {
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
              for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                  const float v = acc[rt][qt][g], fr = fe_s[(2 * wr + rt) * 32 + tile_row_local(g, (int)h)];
                  m_nn[qt] = fminf(m_nn[qt], v);
                  m_hd[qt] = fminf(m_hd[qt], (fr < feq[qt]) ? v : INFINITY);
                }
              // (the two halves of the wave hold other reference rows of the same queries: any minimum met serves both)
              m_nn[qt] = fminf(m_nn[qt], __shfl_xor(m_nn[qt], 32, 64));
              m_hd[qt] = fminf(m_hd[qt], __shfl_xor(m_hd[qt], 32, 64));
              if (h == 0) {
                min_s[wave][qt][0][c] = m_nn[qt];
                min_s[wave][qt][1][c] = m_hd[qt];
              }
            }
            // ... and so do the two waves that hold the other reference tiles of the same queries (wave ^ 2): one search per
            // query and share instead of two.  Every wave of the workgroup is in this epilogue (the chunk count is uniform);
            // the next block's minima are written behind the barrier that closes this chunk.
            __syncthreads();
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
              m_nn[qt] = fminf(m_nn[qt], min_s[wave ^ 2u][qt][0][c]);
              m_hd[qt] = fminf(m_hd[qt], min_s[wave ^ 2u][qt][1][c]);
              const float cut_nn = wide_cut(m_nn[qt], band, ratio), cut_hd = wide_cut(m_hd[qt], band, ratio);
#pragma unroll
              for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                  const float v = acc[rt][qt][g], fr = fe_s[(2 * wr + rt) * 32 + tile_row_local(g, (int)h)];
                  const uint32_t fl = ((v <= cut_nn) ? 1u : 0u) | (((fr < feq[qt]) & (v <= cut_hd)) ? 2u : 0u);
                  if ((__builtin_amdgcn_ballot_w64(fl != 0) & livemask[qt]) != 0) {
                    // (kFresh: the sixteen row offsets 4 h | k of a tile are otherwise kept in a register each, across the sweep)
                    const uint32_t i = (rb * kWideBlockTiles + 2 * wr + rt) * 32 + tile_row_local(g, (int)wide_fresh<kFresh>(h));
                    push(fl != 0 && live[qt] && i < X.n_rows && (SM == kAgainst || i != jq[qt]), i, ((2 * wq + qt) * 32 + c) | (fl << 8));
                  }
                }
            }
          }
        }
        if (it + 1 < n_run) store(it + 1);
        __syncthreads();
      }
    }
    round0 += kWideListCap;
  } while (PR && round0 < nblk);

  if constexpr (MODE != kWideDump) {
    if (fill != 0) {
      drain();
      n_exact += fill;
    }
  }
  if constexpr (MODE == kWidePairs) {
    if (lane == 0 && n_found != 0) atomicAdd(X.count, n_found);
  }
  if constexpr (MODE == kWideMinEdge) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      // (the two halves of the wave hold other reference rows of the same queries)
      const uint32_t m = min(rmin[qt], (uint32_t)__shfl_xor((int)rmin[qt], 32, 64));
      if (h == 0 && live[qt] && m != ~0u)
        atomicMin(&X.best[comp_q[qt]], ((unsigned long long)max(rank_q[qt], m) << 32) | min(rank_q[qt], m));
    }
  }
  if constexpr (kCount) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        const uint32_t total = cnt[qt][k] + (uint32_t)__shfl_xor((int)cnt[qt][k], 32, 64);
        // the frame itself: the 1 the reference starts every population at, added once per row
        const uint32_t add = total + ((SM == kSelf && y == 0 && wr == 0) ? 1u : 0u);
        if (h == 0 && live[qt] && k < X.n_rad && add != 0) atomicAdd(&X.pops[(size_t)k * n_q + jq[qt]], add);
      }
  }
  if (lane == 0 && n_exact != 0) atomicAdd(reinterpret_cast<unsigned long long*>(X.hdr + kWideHdrExact), n_exact);
  if (tid == 0) {
    const unsigned long long tiles = (unsigned long long)n_eval * kWideBlockTiles * kWideBlockTiles;
    atomicAdd(reinterpret_cast<unsigned long long*>(X.hdr + kWideHdrTiles), tiles);
    atomicAdd(reinterpret_cast<unsigned long long*>(X.hdr + kWideHdrMfma), tiles * NM);
  }
}

// the merged words of the rows [i_from, i_to) -> the four outputs ("none" stays where nothing was found)
__global__ void wide_nn_finish_kernel(const uint32_t* __restrict__ hdr, const unsigned long long* __restrict__ merge,
                                      uint32_t n_rows, uint32_t i_from, uint32_t i_to, uint32_t* __restrict__ nn_idx,
                                      float* __restrict__ nn_d2, uint32_t* __restrict__ hd_idx, float* __restrict__ hd_d2) {
  if (hdr[1] != 0) return;
  const uint32_t j = i_from + blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= i_to) return;
  const unsigned long long a = merge[j], b = merge[(size_t)n_rows + j];
  if (a != ~0ull) {
    nn_idx[j] = (uint32_t)a;
    nn_d2[j] = __uint_as_float((uint32_t)(a >> 32));
  }
  if (b != ~0ull) {
    hd_idx[j] = (uint32_t)b;
    hd_d2[j] = __uint_as_float((uint32_t)(b >> 32));
  }
}

}  // namespace

}  // namespace dc
