// dc_direct.hip -- exact-by-construction VALU kernels of the density hot path (gfx950).
//
// Replaces the reference's CUDA kernels population_count
// (density_clustering_cuda_kernels.cu:9-56) and nearest_neighbor_search (:58-130), but with the
// arithmetic and the decision rules of the reference's CPU path (density_clustering.cpp:126-288),
// which is the parity target: strict '<', duplicates are neighbours, lowest index wins ties,
// "none" = (n_rows+1, FLT_MAX), and d2 in the reference binary's float order (dist2_canon).
//
// Shape (one launch sweeps ALL reference frames; the reference needs ceil(N/512) launches):
//   - a workgroup of 256 lanes owns 256*Q query frames; each lane keeps its Q query rows in
//     VGPRs for the whole sweep (Q*D registers);
//   - reference frames stream through one LDS tile of 256 rows (row stride padded to a
//     multiple of 4 floats so that a row is read with ds_read_b128); every lane of a wave reads
//     the SAME row -> LDS broadcast, no bank conflicts;
//   - coordinates are read row-major and fully coalesced from HBM/L2 (a tile is one contiguous
//     256*D*4-byte span);
//   - counters / running minima are per-lane registers, so no cross-lane reduction is needed.
// VALU-bound by design: 3D-1 non-fusable float ops per pair (no FMA is allowed by the spec).
#include "dc_common.hpp"

#include <float.h>
#include <array>
#include <utility>

namespace dc {

namespace {

constexpr int kBlock = 256;   // lanes per workgroup (4 waves: one per SIMD)
constexpr int kTile = 256;    // reference frames per LDS tile

template <int D>
struct Cfg {
  static constexpr int S = (D + 3) & ~3;                       // LDS row stride (floats)
  static constexpr int Q = (D <= 12) ? 4 : (D <= 24 ? 2 : 1);  // query rows per lane
};

// contiguous span of nt rows -> padded LDS tile
template <int D>
__device__ __forceinline__ void stage_tile(const float* __restrict__ coords, uint32_t t0,
                                           uint32_t nt, float* tile) {
  constexpr int S = Cfg<D>::S;
  const float* src = coords + (size_t)t0 * D;
  const uint32_t ne = nt * D;
  for (uint32_t e = threadIdx.x; e < ne; e += kBlock) {
    const uint32_t row = e / D, col = e - row * D;
    tile[row * S + col] = src[e];
  }
}

template <int D>
__device__ __forceinline__ void load_ref(const float* tile, uint32_t r, float (&ref)[D]) {
  constexpr int S = Cfg<D>::S;
  const float4* r4 = reinterpret_cast<const float4*>(tile + r * S);
#pragma unroll
  for (int m = 0; m < S / 4; ++m) {
    const float4 v = r4[m];
    if (4 * m + 0 < D) ref[4 * m + 0] = v.x;
    if (4 * m + 1 < D) ref[4 * m + 1] = v.y;
    if (4 * m + 2 < D) ref[4 * m + 2] = v.z;
    if (4 * m + 3 < D) ref[4 * m + 3] = v.w;
  }
}

// -----------------------------------------------------------------------------------------
// The query rows [i_from, i_to) of qcoords [n_q][D] against every row of rcoords [n_ref][D].  M decides
// the rest:
//   kSelf (qcoords == rcoords, n_q == n_ref): the reference's sweep, which leaves out the self pair:
//     pops[r][i] = 1 + #{ j != i : d2(i,j) < rad2[r] };  nn / hd over j != i
//   kAgainst: nothing is left out and nothing is added (dc_hip_*_cross_dev):
//     pops[r][q] = #{ j < n_ref : d2(Q_q, R_j) < rad2[r] };  nn / hd over every j;  fe_q == nullptr: nn only
// "none" is (n_ref + 1, FLT_MAX) in both.
// -----------------------------------------------------------------------------------------
template <int D, int NR, SweepMode M>
__global__ __launch_bounds__(kBlock) void pop_direct_kernel(
    const float* __restrict__ qcoords, const float* __restrict__ rcoords, uint32_t n_q, uint32_t n_ref,
    uint32_t i_from, uint32_t i_to, Rad2 rad2, int n_rad, uint32_t* __restrict__ pops,
    const uint32_t* __restrict__ gate) {
  constexpr int S = Cfg<D>::S, Q = Cfg<D>::Q;
  if (gate && gate[1] == 0) return;
  if constexpr (M == kSelf) rcoords = qcoords, n_q = n_ref;   // (one array: the registers of the reference's loop)
  __shared__ __attribute__((aligned(16))) float tile[kTile * S];
  const uint32_t qbase = i_from + blockIdx.x * (kBlock * Q);

  float q[Q][D];
  uint32_t qi[Q];
#pragma unroll
  for (int a = 0; a < Q; ++a) {
    qi[a] = qbase + a * kBlock + threadIdx.x;
    const uint32_t row = qi[a] < i_to ? qi[a] : i_to - 1;   // clamp: result discarded
#pragma unroll
    for (int k = 0; k < D; ++k) q[a][k] = qcoords[(size_t)row * D + k];
  }
  uint32_t cnt[Q][NR];
#pragma unroll
  for (int a = 0; a < Q; ++a)
#pragma unroll
    for (int r = 0; r < NR; ++r) cnt[a][r] = 0;

  for (uint32_t t0 = 0; t0 < n_ref; t0 += kTile) {
    const uint32_t nt = min((uint32_t)kTile, n_ref - t0);
    __syncthreads();
    stage_tile<D>(rcoords, t0, nt, tile);
    __syncthreads();
#pragma unroll 2
    for (uint32_t r = 0; r < nt; ++r) {
      float ref[D];
      load_ref<D>(tile, r, ref);
#pragma unroll
      for (int a = 0; a < Q; ++a) {
        const float d = dist2_canon<D>(q[a], ref);
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) cnt[a][rr] += (d < rad2.v[rr]) ? 1u : 0u;
      }
    }
  }
  // A self sweep counted the self pair iff d2(i,i) < rad2 (d2(i,i) is +0, or NaN for non-finite
  // rows); the reference never evaluates it and starts every population at 1 (:132-134).
#pragma unroll
  for (int a = 0; a < Q; ++a) {
    if (qi[a] < i_to) {
      const float dself = (M == kSelf) ? dist2_canon<D>(q[a], q[a]) : 0.0f;
#pragma unroll
      for (int rr = 0; rr < NR; ++rr)
        if (rr < n_rad)   // an instance with NR slots also serves fewer radii (unused slots = -1)
          pops[(size_t)rr * n_q + qi[a]] =
              (M == kSelf) ? cnt[a][rr] + 1u - ((dself < rad2.v[rr]) ? 1u : 0u) : cnt[a][rr];
    }
  }
}

// -----------------------------------------------------------------------------------------
// nearest neighbour / nearest neighbour with lower free energy
// -----------------------------------------------------------------------------------------
template <int D, int Q, bool DIAG>
__device__ __forceinline__ void nn_tile(const float* tile, const float* tile_fe, uint32_t t0,
                                        uint32_t nt, const float (&q)[Q][D],
                                        const uint32_t (&qi)[Q], const float (&qfe)[Q],
                                        float (&best)[Q], uint32_t (&bj)[Q], float (&bhd)[Q],
                                        uint32_t (&bjhd)[Q]) {
#pragma unroll 2
  for (uint32_t r = 0; r < nt; ++r) {
    float ref[D];
    load_ref<D>(tile, r, ref);
    const float rfe = tile_fe[r];
    const uint32_t j = t0 + r;
#pragma unroll
    for (int a = 0; a < Q; ++a) {
      const float d = dist2_canon<D>(q[a], ref);
      bool lt = d < best[a];                       // strict: first (lowest) j wins ties, :270
      bool lh = (rfe < qfe[a]) && (d < bhd[a]);    // :275-276
      if (DIAG) {
        const bool other = (j != qi[a]);           // :262
        lt = lt && other;
        lh = lh && other;
      }
      best[a] = lt ? d : best[a];
      bj[a] = lt ? j : bj[a];
      bhd[a] = lh ? d : bhd[a];
      bjhd[a] = lh ? j : bjhd[a];
    }
  }
}

template <int D, SweepMode M>
__global__ __launch_bounds__(kBlock) void nn_direct_kernel(
    const float* __restrict__ qcoords, const float* __restrict__ rcoords, uint32_t n_ref,
    const float* __restrict__ fe_q, const float* __restrict__ fe_r, uint32_t i_from, uint32_t i_to,
    uint32_t* __restrict__ nn_idx, float* __restrict__ nn_d2, uint32_t* __restrict__ hd_idx,
    float* __restrict__ hd_d2, const uint32_t* __restrict__ gate) {
  constexpr int S = Cfg<D>::S, Q = Cfg<D>::Q;
  if (gate && gate[1] == 0) return;
  __shared__ __attribute__((aligned(16))) float tile[kTile * S];
  __shared__ float tile_fe[kTile];
  const uint32_t qbase = i_from + blockIdx.x * (kBlock * Q);
  const uint32_t qend = min(qbase + kBlock * Q, i_to);   // this workgroup's rows: [qbase, qend)
  if constexpr (M == kSelf) rcoords = qcoords, fe_r = fe_q;
  const bool with_fe = (M == kSelf) || fe_q;            // (a self sweep always has free energies)

  float q[Q][D], qfe[Q], best[Q], bhd[Q];
  uint32_t qi[Q], bj[Q], bjhd[Q];
#pragma unroll
  for (int a = 0; a < Q; ++a) {
    qi[a] = qbase + a * kBlock + threadIdx.x;
    const uint32_t row = qi[a] < i_to ? qi[a] : i_to - 1;
#pragma unroll
    for (int k = 0; k < D; ++k) q[a][k] = qcoords[(size_t)row * D + k];
    qfe[a] = with_fe ? fe_q[row] : -INFINITY;   // (no free energies: nothing is lower)
    best[a] = FLT_MAX;       // :257-260
    bhd[a] = FLT_MAX;
    bj[a] = n_ref + 1;
    bjhd[a] = n_ref + 1;
  }

  for (uint32_t t0 = 0; t0 < n_ref; t0 += kTile) {
    const uint32_t nt = min((uint32_t)kTile, n_ref - t0);
    __syncthreads();
    stage_tile<D>(rcoords, t0, nt, tile);
    if (threadIdx.x < nt) tile_fe[threadIdx.x] = with_fe ? fe_r[t0 + threadIdx.x] : 0.0f;
    __syncthreads();
    // only tiles that overlap this workgroup's own rows can contain a self pair
    if (M == kSelf && t0 < qend && t0 + nt > qbase)
      nn_tile<D, Q, true>(tile, tile_fe, t0, nt, q, qi, qfe, best, bj, bhd, bjhd);
    else
      nn_tile<D, Q, false>(tile, tile_fe, t0, nt, q, qi, qfe, best, bj, bhd, bjhd);
  }
#pragma unroll
  for (int a = 0; a < Q; ++a) {
    if (qi[a] < i_to) {
      nn_idx[qi[a]] = bj[a];
      nn_d2[qi[a]] = best[a];
      if (with_fe) {
        hd_idx[qi[a]] = bjhd[a];
        hd_d2[qi[a]] = bhd[a];
      }
    }
  }
}

// -----------------------------------------------------------------------------------------
// generic n_cols (33..kMaxColsGeneric): query rows live in LDS, lane-major ([k][lane], no bank
// conflicts); 64 lanes per workgroup, 32 reference rows per tile.  Same arithmetic, same modes.
// -----------------------------------------------------------------------------------------
constexpr int kGBlock = 64, kGTile = 32;

template <SweepMode M>
__global__ __launch_bounds__(kGBlock) void pop_generic_kernel(
    const float* __restrict__ qcoords, const float* __restrict__ rcoords, uint32_t n_q, uint32_t n_ref,
    uint32_t D, uint32_t i_from, uint32_t i_to, Rad2 rad2, int n_rad, uint32_t* __restrict__ pops,
    const uint32_t* __restrict__ gate) {
  if (gate && gate[1] == 0) return;
  if constexpr (M == kSelf) rcoords = qcoords, n_q = n_ref;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* qs = smem;                        // [D][kGBlock]
  float* tile = smem + (size_t)D * kGBlock;  // [kGTile][D]
  const uint32_t qi = i_from + blockIdx.x * kGBlock + threadIdx.x;
  const uint32_t row = qi < i_to ? qi : i_to - 1;
  for (uint32_t k = 0; k < D; ++k) qs[k * kGBlock + threadIdx.x] = qcoords[(size_t)row * D + k];
  uint32_t cnt[kMaxRadiiPerLaunch];
#pragma unroll
  for (int r = 0; r < kMaxRadiiPerLaunch; ++r) cnt[r] = 0;
  for (uint32_t t0 = 0; t0 < n_ref; t0 += kGTile) {
    const uint32_t nt = min((uint32_t)kGTile, n_ref - t0);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nt * D; e += kGBlock) tile[e] = rcoords[(size_t)t0 * D + e];
    __syncthreads();
    for (uint32_t r = 0; r < nt; ++r) {
      const float d = dist2_canon_rt(qs + threadIdx.x, kGBlock, tile + r * D, 1, (int)D);
#pragma unroll
      for (int rr = 0; rr < kMaxRadiiPerLaunch; ++rr) cnt[rr] += (d < rad2.v[rr]) ? 1u : 0u;
    }
  }
  if (qi < i_to) {
    const float dself =
        (M == kSelf) ? dist2_canon_rt(qs + threadIdx.x, kGBlock, qs + threadIdx.x, kGBlock, (int)D) : 0.0f;
#pragma unroll
    for (int rr = 0; rr < kMaxRadiiPerLaunch; ++rr)
      if (rr < n_rad)
        pops[(size_t)rr * n_q + qi] = (M == kSelf) ? cnt[rr] + 1u - ((dself < rad2.v[rr]) ? 1u : 0u) : cnt[rr];
  }
}

template <SweepMode M>
__global__ __launch_bounds__(kGBlock) void nn_generic_kernel(
    const float* __restrict__ qcoords, const float* __restrict__ rcoords, uint32_t n_ref, uint32_t D,
    const float* __restrict__ fe_q, const float* __restrict__ fe_r, uint32_t i_from, uint32_t i_to,
    uint32_t* __restrict__ nn_idx, float* __restrict__ nn_d2, uint32_t* __restrict__ hd_idx,
    float* __restrict__ hd_d2, const uint32_t* __restrict__ gate) {
  if (gate && gate[1] == 0) return;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* qs = smem;
  float* tile = smem + (size_t)D * kGBlock;
  float* tile_fe = tile + (size_t)kGTile * D;
  if constexpr (M == kSelf) rcoords = qcoords, fe_r = fe_q;
  const bool with_fe = (M == kSelf) || fe_q;
  const uint32_t qi = i_from + blockIdx.x * kGBlock + threadIdx.x;
  const uint32_t row = qi < i_to ? qi : i_to - 1;
  for (uint32_t k = 0; k < D; ++k) qs[k * kGBlock + threadIdx.x] = qcoords[(size_t)row * D + k];
  const float qfe = with_fe ? fe_q[row] : -INFINITY;
  float best = FLT_MAX, bhd = FLT_MAX;
  uint32_t bj = n_ref + 1, bjhd = n_ref + 1;
  for (uint32_t t0 = 0; t0 < n_ref; t0 += kGTile) {
    const uint32_t nt = min((uint32_t)kGTile, n_ref - t0);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nt * D; e += kGBlock) tile[e] = rcoords[(size_t)t0 * D + e];
    if (threadIdx.x < nt) tile_fe[threadIdx.x] = with_fe ? fe_r[t0 + threadIdx.x] : 0.0f;
    __syncthreads();
    for (uint32_t r = 0; r < nt; ++r) {
      const uint32_t j = t0 + r;
      const float d = dist2_canon_rt(qs + threadIdx.x, kGBlock, tile + r * D, 1, (int)D);
      const bool other = (M != kSelf) || (j != qi);
      const bool lt = other && (d < best);
      const bool lh = other && (tile_fe[r] < qfe) && (d < bhd);
      best = lt ? d : best;
      bj = lt ? j : bj;
      bhd = lh ? d : bhd;
      bjhd = lh ? j : bjhd;
    }
  }
  if (qi < i_to) {
    nn_idx[qi] = bj;
    nn_d2[qi] = best;
    if (with_fe) {
      hd_idx[qi] = bjhd;
      hd_d2[qi] = bhd;
    }
  }
}

// -----------------------------------------------------------------------------------------
// radius graph (canonical d2 < r2, the graph of the reference's screening, density_clustering.cpp:
// 292-332) for every n_cols the sweeps above accept: the two products of the matrix-core sweep's
// sinks (dc_mfma.hpp EdgeSink), for n_cols > 64 and for data the operand-image pass flagged.
// Same tiles and arithmetic as the population kernels, whose output they write as well.
//   kGraphPairs:   every unordered pair {i, j} once, from its query i < j.  Hits go into a wave-private
//                  LDS queue (ballot + mbcnt) that is flushed with ONE 64-bit atomicAdd per batch;
//                  capacity 0 counts only (the flushes still add to the count)
//   kGraphMinEdge: per query the lightest (max(rank) << 32 | min(rank)) over the partners of another
//                  component, then one 64-bit atomicMin into best[comp[i]] (a Boruvka round)
// -----------------------------------------------------------------------------------------
enum GraphMode { kGraphPairs = 1, kGraphMinEdge = 2 };
template <int D, int Q, int MODE>
__device__ __forceinline__ void graph_tile(const float* tile, const uint32_t* tile_cr, uint32_t t0, uint32_t nt,
                                           bool emit, float r2, const float (&q)[Q][D], const uint32_t (&qi)[Q],
                                           const bool (&live)[Q], const uint32_t (&qc)[Q], const uint32_t (&qr)[Q],
                                           uint32_t (&cnt)[Q], unsigned long long (&best)[Q], uint2* queue,
                                           uint32_t& fill, const GraphOut& g) {
  auto row = [&](uint32_t r) {
    float ref[D];
    load_ref<D>(tile, r, ref);
    const uint32_t j = t0 + r;
#pragma unroll
    for (int a = 0; a < Q; ++a) {
      const float d = dist2_canon<D>(q[a], ref);
      const bool hit = d < r2;
      cnt[a] += hit ? 1u : 0u;
      if constexpr (MODE == kGraphMinEdge) {
        // (the self pair and every pair inside the component: same id)
        const uint32_t rr = tile_cr[kTile + r];
        const unsigned long long key = ((unsigned long long)max(qr[a], rr) << 32) | min(qr[a], rr);
        best[a] = (hit && tile_cr[r] != qc[a] && key < best[a]) ? key : best[a];
      } else {
        if (emit) pair_push(hit && live[a] && j > qi[a], qi[a], j, queue, fill, g);
      }
    }
  };
  if constexpr (MODE == kGraphMinEdge) {
#pragma unroll 2
    for (uint32_t r = 0; r < nt; ++r) row(r);
  } else {   // (a flush inside the body: no unrolling)
    for (uint32_t r = 0; r < nt; ++r) row(r);
  }
}

template <int D, int MODE>
__global__ __launch_bounds__(kBlock) void graph_direct_kernel(const float* __restrict__ coords, uint32_t n_rows,
                                                              uint32_t i_from, uint32_t i_to, float r2, GraphOut g,
                                                              const uint32_t* __restrict__ gate) {
  constexpr int S = Cfg<D>::S, Q = Cfg<D>::Q;
  constexpr bool kMin = MODE == kGraphMinEdge;
  if (gate && gate[1] == 0) return;
  __shared__ __attribute__((aligned(16))) float tile[kTile * S];
  __shared__ uint32_t tile_cr[kMin ? 2 * kTile : 1];                  // comp, rank of the tile's rows
  __shared__ uint2 queues[kMin ? 1 : (kBlock / 64) * kPairQueue];    // one pair queue per wave
  uint2* queue = queues + (kMin ? 0u : (threadIdx.x >> 6) * kPairQueue);
  const uint32_t qbase = i_from + blockIdx.x * (kBlock * Q);
  const uint32_t wave_lo = qbase + (threadIdx.x & ~63u);   // this wave's lowest query row

  float q[Q][D];
  uint32_t qi[Q], cnt[Q], qc[Q], qr[Q];
  bool live[Q];
  unsigned long long best[Q];
#pragma unroll
  for (int a = 0; a < Q; ++a) {
    qi[a] = qbase + a * kBlock + threadIdx.x;
    live[a] = qi[a] < i_to;
    const uint32_t row = live[a] ? qi[a] : i_to - 1;   // clamp: result discarded
#pragma unroll
    for (int k = 0; k < D; ++k) q[a][k] = coords[(size_t)row * D + k];
    cnt[a] = 0;
    qc[a] = kMin ? g.comp[row] : 0u;
    qr[a] = kMin ? g.rank[row] : 0u;
    best[a] = ~0ull;
  }
  uint32_t fill = 0;
  for (uint32_t t0 = 0; t0 < n_rows; t0 += kTile) {
    const uint32_t nt = min((uint32_t)kTile, n_rows - t0);
    __syncthreads();
    stage_tile<D>(coords, t0, nt, tile);
    if (kMin && threadIdx.x < nt) {
      tile_cr[threadIdx.x] = g.comp[t0 + threadIdx.x];
      tile_cr[kTile + threadIdx.x] = g.rank[t0 + threadIdx.x];
    }
    __syncthreads();
    // a pair is listed from its lower row: tiles wholly at or below the wave's rows list nothing
    graph_tile<D, Q, MODE>(tile, tile_cr, t0, nt, t0 + nt > wave_lo + 1u, r2, q, qi, live, qc, qr, cnt, best, queue,
                           fill, g);
  }
  if constexpr (!kMin) {
    if (fill) pair_flush(queue, fill, g);
  }
#pragma unroll
  for (int a = 0; a < Q; ++a) {
    if (live[a]) {
      const float dself = dist2_canon<D>(q[a], q[a]);   // (see pop_direct_kernel)
      g.pops[qi[a]] = cnt[a] + 1u - ((dself < r2) ? 1u : 0u);
      if (kMin && best[a] != ~0ull) atomicMin(g.best + qc[a], best[a]);
    }
  }
}

// generic n_cols: the layout of pop_generic_kernel, then [2][kGTile] comp / rank (min edge) or the wave's pair queue
template <int MODE>
__global__ __launch_bounds__(kGBlock) void graph_generic_kernel(const float* __restrict__ coords, uint32_t n_rows,
                                                                uint32_t D, uint32_t i_from, uint32_t i_to, float r2,
                                                                GraphOut g, const uint32_t* __restrict__ gate) {
  constexpr bool kMin = MODE == kGraphMinEdge;
  if (gate && gate[1] == 0) return;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* qs = smem;                          // [D][kGBlock]
  float* tile = smem + (size_t)D * kGBlock;  // [kGTile][D]
  uint32_t* tile_cr = reinterpret_cast<uint32_t*>(tile + (size_t)kGTile * D);
  uint2* queue = reinterpret_cast<uint2*>(tile + (size_t)kGTile * D);
  const uint32_t wave_lo = i_from + blockIdx.x * kGBlock;
  const uint32_t qi = wave_lo + threadIdx.x;
  const bool live = qi < i_to;
  const uint32_t row = live ? qi : i_to - 1;
  for (uint32_t k = 0; k < D; ++k) qs[k * kGBlock + threadIdx.x] = coords[(size_t)row * D + k];
  const uint32_t qc = kMin ? g.comp[row] : 0u, qr = kMin ? g.rank[row] : 0u;
  uint32_t cnt = 0, fill = 0;
  unsigned long long best = ~0ull;
  for (uint32_t t0 = 0; t0 < n_rows; t0 += kGTile) {
    const uint32_t nt = min((uint32_t)kGTile, n_rows - t0);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nt * D; e += kGBlock) tile[e] = coords[(size_t)t0 * D + e];
    if (kMin && threadIdx.x < nt) {
      tile_cr[threadIdx.x] = g.comp[t0 + threadIdx.x];
      tile_cr[kGTile + threadIdx.x] = g.rank[t0 + threadIdx.x];
    }
    __syncthreads();
    const bool emit = t0 + nt > wave_lo + 1u;
    for (uint32_t r = 0; r < nt; ++r) {
      const uint32_t j = t0 + r;
      const float d = dist2_canon_rt(qs + threadIdx.x, kGBlock, tile + r * D, 1, (int)D);
      const bool hit = d < r2;
      cnt += hit ? 1u : 0u;
      if constexpr (kMin) {
        const uint32_t rr = tile_cr[kGTile + r];
        const unsigned long long key = ((unsigned long long)max(qr, rr) << 32) | min(qr, rr);
        best = (hit && tile_cr[r] != qc && key < best) ? key : best;
      } else {
        if (emit) pair_push(hit && live && j > qi, qi, j, queue, fill, g);
      }
    }
  }
  if constexpr (!kMin) {
    if (fill) pair_flush(queue, fill, g);
  }
  if (live) {
    const float dself = dist2_canon_rt(qs + threadIdx.x, kGBlock, qs + threadIdx.x, kGBlock, (int)D);
    g.pops[qi] = cnt + 1u - ((dself < r2) ? 1u : 0u);
    if (kMin && best != ~0ull) atomicMin(g.best + qc, best);
  }
}

// -----------------------------------------------------------------------------------------
// small helpers
// -----------------------------------------------------------------------------------------
// every query row starts at "none" = (none, FLT_MAX) (density_clustering.cpp:242-245); hd may be absent (nn only)
__global__ void nn_init_kernel(uint32_t n_q, uint32_t none, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx,
                               float* hd_d2) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_q) {
    nn_idx[i] = none;
    nn_d2[i] = FLT_MAX;
    if (hd_idx) {
      hd_idx[i] = none;
      hd_d2[i] = FLT_MAX;
    }
  }
}

__global__ void fe_gather_kernel(const uint32_t* __restrict__ pops, uint32_t n_rows,
                                 const float* __restrict__ table, float* __restrict__ fe) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_rows) fe[i] = table[pops[i]];
}

// Free energies on the device, with the host libm as the referee.  The reference computes
// fe = (float)(-log((double)((float)pop * (1.0f / max_pop)))) with glibc's double log
// (density_clustering.cpp:201-209 as compiled).  The device's double log differs from
// it by at most a few ulp(double); the two can only round to different floats when the double value lies
// within that distance of a float rounding boundary (a midpoint of neighbouring floats).  Such rows -- one
// in 2^22 with the margin below -- are listed for the host, which recomputes them with its libm.
// q, the reciprocal (double division rounded to float = correctly rounded float division, 53 >= 2*24+2)
// and the final rounding are IEEE operations, identical on both sides.
// state (device, kFeStateWords words): two slots of (max population, number of listed rows) used by alternate calls --
// slot = call parity.  The slot of the NEXT call is cleared by this call's kernel (its first thread), so that a step needs
// no fill kernels: max_u32_kernel and the rows' atomicAdd start from zeros.  (A first version cleared its own slot from
// the last block to finish, found with a ticket behind a __threadfence(): 245 us instead of 7 -- a device-scope release
// per block is an L2 write-back per block.)
__global__ void fe_log_kernel(const uint32_t* __restrict__ pops, uint32_t n_rows, uint32_t* __restrict__ state, uint32_t slot,
                              float* __restrict__ fe, uint2* __restrict__ flag_list, uint32_t flag_cap, double tol_rel) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    state[2u * (slot ^ 1u)] = 0u;
    state[2u * (slot ^ 1u) + 1u] = 0u;
  }
  if (i >= n_rows) return;
  const float rec = (float)(1.0 / (double)(float)(state[2u * slot]));
  const uint32_t pop = pops[i];
  const float q = (float)pop * rec;
  const double y = -log((double)q);
  const float f = (float)y;
  fe[i] = f;
  if (fabs(y) <= 1.0e300 && y != 0.0) {
    const uint32_t fb = __float_as_uint(f);
    // neighbours of f by magnitude (f != 0, finite: fe is at most -log(2^-24 / 1) = 16.6)
    const double up = (double)__uint_as_float(fb + 1u), dn = (double)__uint_as_float(fb - 1u);
    const double tol = tol_rel * fabs(y);   // default 64 ulp(double): device log <= 2 ulp, glibc log <= 1 ulp
    if (fabs(y - 0.5 * ((double)f + up)) < tol || fabs(y - 0.5 * ((double)f + dn)) < tol) {
      const uint32_t k = atomicAdd(state + 2u * slot + 1u, 1u);
      if (k < flag_cap) flag_list[k] = make_uint2(i, pop);
    }
  }
}

// neighbour results as order-preserving 64-bit words (d2 bits << 32 | index): d2 >= 0, so the words of a
// row order like the lexicographic (d2, index) and partial results merge with an integer minimum
__global__ void nn_pack_kernel(const uint32_t* __restrict__ nn_idx, const float* __restrict__ nn_d2,
                               const uint32_t* __restrict__ hd_idx, const float* __restrict__ hd_d2,
                               uint32_t n_rows, unsigned long long* __restrict__ words) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  words[i] = ((unsigned long long)__float_as_uint(nn_d2[i]) << 32) | nn_idx[i];
  words[(size_t)n_rows + i] = ((unsigned long long)__float_as_uint(hd_d2[i]) << 32) | hd_idx[i];
}
__global__ void nn_unpack_kernel(const unsigned long long* __restrict__ words, uint32_t n_rows,
                                 uint32_t* __restrict__ nn_idx, float* __restrict__ nn_d2,
                                 uint32_t* __restrict__ hd_idx, float* __restrict__ hd_d2) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const unsigned long long a = words[i], b = words[(size_t)n_rows + i];
  nn_idx[i] = (uint32_t)a;
  nn_d2[i] = __uint_as_float((uint32_t)(a >> 32));
  hd_idx[i] = (uint32_t)b;
  hd_d2[i] = __uint_as_float((uint32_t)(b >> 32));
}

__global__ void max_u32_kernel(const uint32_t* __restrict__ v, uint32_t n, uint32_t* out) {
  __shared__ uint32_t wave_max[4];
  uint32_t m = 0;
  // 16 bytes per lane and step (cudaMalloc-aligned arrays; the tail by the word)
  const uint32_t n4 = ((reinterpret_cast<uintptr_t>(v) & 15u) == 0) ? n / 4 : 0;
  const uint4* v4 = reinterpret_cast<const uint4*>(v);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
    const uint4 w = v4[i];
    m = max(max(m, max(w.x, w.y)), max(w.z, w.w));
  }
  for (uint32_t i = 4 * n4 + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) m = max(m, v[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  // one atomic per block, and only if it can raise the word (thousands of atomics on one word serialise: 35 us at 10^6 rows)
  if (threadIdx.x == 0) {
    m = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
    if (m > __atomic_load_n(out, __ATOMIC_RELAXED)) atomicMax(out, m);
  }
}

// ---- dispatch tables over n_cols ---------------------------------------------------------
using PopLaunch = void (*)(const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, const Rad2&, int,
                           uint32_t*, const uint32_t*, hipStream_t);
using NnLaunch = void (*)(const float*, const float*, uint32_t, const float*, const float*, uint32_t, uint32_t,
                          uint32_t*, float*, uint32_t*, float*, const uint32_t*, hipStream_t);

template <int D, int NR, SweepMode M>
void pop_launch(const float* qc, const float* rc, uint32_t n_q, uint32_t n_ref, uint32_t i_from, uint32_t i_to,
                const Rad2& rad2, int n_rad, uint32_t* pops, const uint32_t* gate, hipStream_t s) {
  const uint32_t per_block = kBlock * Cfg<D>::Q;
  const uint32_t grid = (i_to - i_from + per_block - 1) / per_block;
  hipLaunchKernelGGL((pop_direct_kernel<D, NR, M>), dim3(grid), dim3(kBlock), 0, s, qc, rc, n_q, n_ref, i_from, i_to,
                     rad2, n_rad, pops, gate);
}

template <int D, SweepMode M>
void nn_launch(const float* qc, const float* rc, uint32_t n_ref, const float* fe_q, const float* fe_r,
               uint32_t i_from, uint32_t i_to, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx, float* hd_d2,
               const uint32_t* gate, hipStream_t s) {
  const uint32_t per_block = kBlock * Cfg<D>::Q;
  const uint32_t grid = (i_to - i_from + per_block - 1) / per_block;
  hipLaunchKernelGGL((nn_direct_kernel<D, M>), dim3(grid), dim3(kBlock), 0, s, qc, rc, n_ref, fe_q, fe_r, i_from,
                     i_to, nn_idx, nn_d2, hd_idx, hd_d2, gate);
}

template <int NR, SweepMode M, int... Ds>
constexpr auto make_pop_table(std::integer_sequence<int, Ds...>) {
  return std::array<PopLaunch, sizeof...(Ds)>{&pop_launch<Ds + 1, NR, M>...};
}
template <SweepMode M, int... Ds>
constexpr auto make_nn_table(std::integer_sequence<int, Ds...>) {
  return std::array<NnLaunch, sizeof...(Ds)>{&nn_launch<Ds + 1, M>...};
}

using DSeq = std::make_integer_sequence<int, kMaxColsTemplated>;
template <int NR, SweepMode M>
const auto kPop = make_pop_table<NR, M>(DSeq{});
template <SweepMode M>
const auto kNn = make_nn_table<M>(DSeq{});

using GraphLaunch = void (*)(const float*, uint32_t, uint32_t, uint32_t, float, const GraphOut&, const uint32_t*,
                             hipStream_t);

template <int D, int MODE>
void graph_launch(const float* c, uint32_t n, uint32_t i_from, uint32_t i_to, float r2, const GraphOut& g,
                  const uint32_t* gate, hipStream_t s) {
  const uint32_t per_block = kBlock * Cfg<D>::Q;
  const uint32_t grid = (i_to - i_from + per_block - 1) / per_block;
  hipLaunchKernelGGL((graph_direct_kernel<D, MODE>), dim3(grid), dim3(kBlock), 0, s, c, n, i_from, i_to, r2, g, gate);
}

template <int MODE, int... Ds>
constexpr auto make_graph_table(std::integer_sequence<int, Ds...>) {
  return std::array<GraphLaunch, sizeof...(Ds)>{&graph_launch<Ds + 1, MODE>...};
}

const auto kGraphPairsTab = make_graph_table<kGraphPairs>(DSeq{});
const auto kGraphMinEdgeTab = make_graph_table<kGraphMinEdge>(DSeq{});

// one launch of the radius-graph kernels over query rows [i_from, i_to); false: n_cols unsupported
template <int MODE>
bool launch_graph(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from, uint32_t i_to, float r2,
                  const GraphOut& g, const uint32_t* gate, hipStream_t stream) {
  if (n_cols >= 1 && n_cols <= (uint32_t)kMaxColsTemplated) {
    if (i_to > i_from)
      (MODE == kGraphPairs ? kGraphPairsTab : kGraphMinEdgeTab)[n_cols - 1](d_coords, n_rows, i_from, i_to, r2, g,
                                                                             gate, stream);
    return true;
  }
  if (n_cols > (uint32_t)kMaxColsTemplated && n_cols <= (uint32_t)kMaxColsGeneric) {
    if (i_to <= i_from) return true;
    const uint32_t grid = (i_to - i_from + kGBlock - 1) / kGBlock;
    const size_t smem = sizeof(float) * (size_t)n_cols * (kGBlock + kGTile) +
                        (MODE == kGraphPairs ? sizeof(uint2) * kPairQueue : sizeof(uint32_t) * 2 * kGTile);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(graph_generic_kernel<MODE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    hipLaunchKernelGGL(graph_generic_kernel<MODE>, dim3(grid), dim3(kGBlock), smem, stream, d_coords, n_rows, n_cols,
                       i_from, i_to, r2, g, gate);
    return true;
  }
  return false;
}

template <SweepMode M>
void pop_direct(const float* d_query, const float* d_ref, uint32_t n_q, uint32_t n_ref, uint32_t n_cols,
                uint32_t i_from, uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops, const uint32_t* gate,
                hipStream_t stream) {
  if (n_cols <= (uint32_t)kMaxColsTemplated) {
    // instances exist for 1, 4 and 8 radius slots; unused slots hold -1 ("d < -1" is never true)
    const auto& tab = (n_rad == 1) ? kPop<1, M> : (n_rad <= 4 ? kPop<4, M> : kPop<8, M>);
    tab[n_cols - 1](d_query, d_ref, n_q, n_ref, i_from, i_to, rad2, n_rad, d_pops, gate, stream);
  } else if (n_cols <= (uint32_t)kMaxColsGeneric) {
    const uint32_t grid = (i_to - i_from + kGBlock - 1) / kGBlock;
    const size_t smem = sizeof(float) * (size_t)n_cols * (kGBlock + kGTile);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pop_generic_kernel<M>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    hipLaunchKernelGGL(pop_generic_kernel<M>, dim3(grid), dim3(kGBlock), smem, stream, d_query, d_ref, n_q, n_ref,
                       n_cols, i_from, i_to, rad2, n_rad, d_pops, gate);
  } else if (M == kSelf) {
    launch_pop_wide(d_query, n_q, n_cols, i_from, i_to, rad2, n_rad, d_pops, gate, stream);
  } else {
    launch_pop_cross_wide(d_query, d_ref, n_q, n_ref, n_cols, i_from, i_to, rad2, n_rad, d_pops, gate, stream);
  }
}

template <SweepMode M>
void nn_direct(const float* d_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols, const float* d_fe_q,
               const float* d_fe_r, uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
               uint32_t* d_hd_idx, float* d_hd_d2, const uint32_t* gate, hipStream_t stream) {
  if (n_cols <= (uint32_t)kMaxColsTemplated) {
    kNn<M>[n_cols - 1](d_query, d_ref, n_ref, d_fe_q, d_fe_r, i_from, i_to, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2,
                       gate, stream);
  } else if (n_cols <= (uint32_t)kMaxColsGeneric) {
    const uint32_t grid = (i_to - i_from + kGBlock - 1) / kGBlock;
    const size_t smem = sizeof(float) * ((size_t)n_cols * (kGBlock + kGTile) + kGTile);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nn_generic_kernel<M>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    hipLaunchKernelGGL(nn_generic_kernel<M>, dim3(grid), dim3(kGBlock), smem, stream, d_query, d_ref, n_ref, n_cols,
                       d_fe_q, d_fe_r, i_from, i_to, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, gate);
  } else if (M == kSelf) {
    launch_nn_wide(d_query, n_ref, n_cols, d_fe_q, i_from, i_to, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, gate, stream);
  } else {
    launch_nn_cross_wide(d_query, d_ref, n_ref, n_cols, d_fe_q, d_fe_r, i_from, i_to, d_nn_idx, d_nn_d2, d_hd_idx,
                         d_hd_d2, gate, stream);
  }
}

}  // namespace

bool launch_pop_direct(const float* d_query, const float* d_ref, uint32_t n_q, uint32_t n_ref, uint32_t n_cols,
                       uint32_t i_from, uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops, SweepMode mode,
                       const uint32_t* gate, hipStream_t stream) {
  if (i_to <= i_from || n_rad <= 0 || n_ref == 0) return true;
  if (n_cols == 0) return false;
  (mode == kSelf ? pop_direct<kSelf> : pop_direct<kAgainst>)(d_query, d_ref, n_q, n_ref, n_cols, i_from, i_to, rad2,
                                                             n_rad, d_pops, gate, stream);
  return true;
}

bool launch_nn_direct(const float* d_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols, const float* d_fe_q,
                      const float* d_fe_r, uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
                      uint32_t* d_hd_idx, float* d_hd_d2, SweepMode mode, const uint32_t* gate, hipStream_t stream) {
  if (i_to <= i_from || n_ref == 0) return true;
  if (n_cols == 0) return false;
  (mode == kSelf ? nn_direct<kSelf> : nn_direct<kAgainst>)(d_query, d_ref, n_ref, n_cols, d_fe_q, d_fe_r, i_from,
                                                           i_to, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, gate, stream);
  return true;
}

bool launch_pairs_direct(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2, uint32_t* d_pops,
                         uint2* d_pairs, unsigned long long capacity, unsigned long long* d_count,
                         const uint32_t* gate, hipStream_t stream) {
  if (n_cols > (uint32_t)kMaxColsGeneric) {
    launch_pairs_wide(d_coords, n_rows, n_cols, r2, d_pops, d_pairs, capacity, d_count, gate, stream);
    return true;
  }
  const GraphOut g{d_pops, d_pairs, d_pairs ? capacity : 0ull, d_count, nullptr, nullptr, nullptr};
  return launch_graph<kGraphPairs>(d_coords, n_rows, n_cols, 0, n_rows, r2, g, gate, stream);
}

bool launch_min_edge_direct(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2,
                            const uint32_t* d_comp, const uint32_t* d_rank, uint32_t i_from, uint32_t i_to,
                            unsigned long long* d_best, uint32_t* d_pops, const uint32_t* gate,
                            hipStream_t stream) {
  if (n_cols > (uint32_t)kMaxColsGeneric) {
    launch_min_edge_wide(d_coords, n_rows, n_cols, r2, d_comp, d_rank, i_from, i_to, d_best, d_pops, gate, stream);
    return true;
  }
  const GraphOut g{d_pops, nullptr, 0ull, nullptr, d_comp, d_rank, d_best};
  return launch_graph<kGraphMinEdge>(d_coords, n_rows, n_cols, i_from, i_to, r2, g, gate, stream);
}

void launch_nn_init(uint32_t n_q, uint32_t n_ref, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                    float* d_hd_d2, hipStream_t stream) {
  if (n_q == 0) return;
  hipLaunchKernelGGL(nn_init_kernel, dim3((n_q + 255) / 256), dim3(256), 0, stream, n_q, n_ref + 1, d_nn_idx, d_nn_d2,
                     d_hd_idx, d_hd_d2);
}

void launch_fe_gather(const uint32_t* d_pops, uint32_t n_rows, const float* d_table, float* d_fe,
                      hipStream_t stream) {
  if (n_rows == 0) return;
  hipLaunchKernelGGL(fe_gather_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, stream, d_pops,
                     n_rows, d_table, d_fe);
}

// (the call's slot of the state is zero on entry: see fe_log_kernel)
void launch_fe_log(const uint32_t* d_pops, uint32_t n_rows, uint32_t* d_state, uint32_t slot, float* d_fe, uint32_t* d_flag_list,
                   uint32_t flag_cap, double tol_rel, hipStream_t stream, uint32_t fixed_max) {
  if (n_rows == 0) return;
  const uint32_t grid = min((n_rows + 1023u) / 1024u, 256u);
  if (fixed_max)   // (the scale of another population array: dc_hip_free_energies_scaled_dev)
    (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_state + 2u * slot), (int)fixed_max, 1, stream);
  else
    hipLaunchKernelGGL(max_u32_kernel, dim3(grid), dim3(256), 0, stream, d_pops, n_rows, d_state + 2u * slot);
  hipLaunchKernelGGL(fe_log_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, stream, d_pops, n_rows, d_state, slot, d_fe,
                     (uint2*)d_flag_list, flag_cap, tol_rel);
}

void launch_nn_pack(const uint32_t* d_nn_idx, const float* d_nn_d2, const uint32_t* d_hd_idx,
                    const float* d_hd_d2, uint32_t n_rows, unsigned long long* d_words, hipStream_t stream) {
  if (n_rows == 0) return;
  hipLaunchKernelGGL(nn_pack_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, stream, d_nn_idx, d_nn_d2,
                     d_hd_idx, d_hd_d2, n_rows, d_words);
}
void launch_nn_unpack(const unsigned long long* d_words, uint32_t n_rows, uint32_t* d_nn_idx, float* d_nn_d2,
                      uint32_t* d_hd_idx, float* d_hd_d2, hipStream_t stream) {
  if (n_rows == 0) return;
  hipLaunchKernelGGL(nn_unpack_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, stream, d_words, n_rows,
                     d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2);
}

void launch_max_u32(const uint32_t* d_pops, uint32_t n_rows, uint32_t* d_out, hipStream_t stream) {
  (void)hipMemsetAsync(d_out, 0, sizeof(uint32_t), stream);
  if (n_rows == 0) return;
  const uint32_t grid = min((n_rows + 1023u) / 1024u, 256u);
  hipLaunchKernelGGL(max_u32_kernel, dim3(grid), dim3(256), 0, stream, d_pops, n_rows, d_out);
}

}  // namespace dc
