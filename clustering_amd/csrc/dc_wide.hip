// dc_wide.hip -- exact sweeps for rows wider than kMaxColsGeneric (gfx950): the columns stream through LDS in chunks.
//
// The generic kernels of dc_direct.hip keep all D columns of their query rows in LDS, which stops fitting at
// kMaxColsGeneric.  Here a workgroup of 256 lanes owns kWRows = 64 query rows and walks reference tiles of kWRef rows;
// the columns of both blocks pass through LDS kWChunk at a time, double-buffered, and every lane accumulates a register
// tile of kTQ x kTR (query, reference) pairs: 4 x 4 with the default order's 4 lane sums per pair, 4 x 2 with the
// 8 of avx / fma (64 accumulators either way).
//
// Exactness.  Each pair keeps the kLanes lane sums of the canonical order (dc_common.hpp: 4 for the default order,
// 8 for avx / fma), column k on lane sum k % kLanes.  A chunk starts at a multiple of kWChunk (a multiple of 8), so
// the chunking never moves a column to another lane sum.  The chunks cover the columns [0, V), V = kLanes * (D /
// kLanes); LDS cells of columns >= V hold +0 in both blocks, and adding (0 - 0)^2 = +0 to a lane sum (never -0) leaves
// it unchanged, as does fma(0, 0, a).  After the last chunk of a tile each pair is finished as dist2_canon_rt /
// canon_sum_avx finish it: the lane-sum combination, then the columns [V, D) from a small tail area staged with the
// last chunk.  Packed f32 additions and multiplications round per element, so v_pk_add_f32 / v_pk_mul_f32 keep the
// arithmetic; a fused multiply-add appears only where DC_CANON_ACC fuses (the fma build).
//
// LDS: a row of a chunk is kWStride = kWChunk + 4 floats (9 slots of 16 B), so the distinct rows that one 16-lane group
// of a ds_read_b128 reads (4 query rows, or 4 reference rows each broadcast to 4 lanes) fall on distinct slots.
#include "dc_common.hpp"

#include <float.h>

namespace dc {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4_row __attribute__((ext_vector_type(4), aligned(4)));   // 4 columns of a row (rows are 4-byte aligned)

#ifdef DC_CANON_AVX
constexpr int kLanes = 8;
constexpr int kTR = 2;                     // (8 lane sums per pair: 4 x 4 pairs would need 128 accumulators)
#else
constexpr int kLanes = 4;
constexpr int kTR = 4;
#endif
constexpr int kTQ = 4;                     // pairs per lane: query rows tq + 4a, reference rows tr + 16c
constexpr int kLanePairs = kLanes / 2;     // lane sums per pair as f2
constexpr int kWBlock = 256;               // lanes per workgroup: 4 waves, each 16 query rows x kWRef reference rows
constexpr int kWRows = 64;                 // query rows per workgroup
constexpr int kWRef = 16 * kTR;            // reference rows per tile
constexpr int kWStage = kWRows + kWRef;    // rows of a chunk in LDS: query rows, then reference rows
constexpr int kWChunk = 32;                // columns per LDS chunk: one 128-byte line of a row
constexpr int kWStride = kWChunk + 4;      // LDS row stride (floats)
constexpr int kWTail = 8;                  // tail columns [V, D) per row (fewer than kLanes)
constexpr int kWLoads = kWStage * (kWChunk / 4) / kWBlock;   // 4-column pieces each lane stages per chunk
static_assert(kWStage * (kWChunk / 4) % kWBlock == 0 && 2 * kWStage <= kWBlock, "staging shape");

enum WideMode { kWidePop = 0, kWideNn = 1, kWidePairs = 2, kWideMinEdge = 3 };

struct WideBuf {
  f4 main[kWStage][kWStride / 4];   // query rows, then NEGATED reference rows: columns [c0, c0 + kWChunk)
  f4 tail[kWStage][kWTail / 4];     // columns [V, D) (last chunk of a tile only)
};

struct WideArgs {
  Rad2 rad2;   // pops: radii of this launch; pairs / min edge: rad2.v[0] = r2
  int n_rad;
  const float* fe;   // nn
  uint32_t* nn_idx;
  float* nn_d2;
  uint32_t* hd_idx;
  float* hd_d2;
  GraphOut g;   // g.pops: pops of radius 0 ([n_rad][n_rows] radius-major for kWidePop)
  // cross sweeps (pop / nn): query rows from qcoords, no pair left out, no self term; pops [n_rad][n_q]; fe = the
  // reference's free energies, fe_q the queries' (nullptr: nn only).  Self sweeps: qcoords = coords, cross = 0.
  const float* qcoords;
  const float* fe_q;
  uint32_t n_q;
  int cross;
};

// what one lane stages of a chunk: kWLoads pieces of 4 columns, and 4 tail columns of one row
struct Stage {
  f4 v[kWLoads];
  f4 t;
};

__device__ __forceinline__ void stage_load(const float* __restrict__ coords, const float* __restrict__ qcoords,
                                           uint32_t n_rows, uint32_t D, uint32_t V,
                                           uint32_t qend, uint32_t qbase, uint32_t t0, uint32_t c0, bool last,
                                           Stage& st) {
#pragma unroll
  for (int m = 0; m < kWLoads; ++m) {
    const uint32_t e = threadIdx.x + kWBlock * m, row = e >> 3, col = c0 + 4u * (e & 7u);
    const uint32_t grow = row < kWRows ? qbase + row : t0 + (row - kWRows);
    const bool ok = (row < kWRows ? grow < qend : grow < n_rows) && col < V;   // (V % 4 == 0: all 4 or none)
    const float* src = row < kWRows ? qcoords : coords;
    st.v[m] = ok ? f4(*reinterpret_cast<const f4_row*>(src + (size_t)grow * D + col)) : f4(0.0f);
  }
  if (last && threadIdx.x < 2 * kWStage) {
    const uint32_t row = threadIdx.x >> 1, k0 = V + 4u * (threadIdx.x & 1u);
    const uint32_t grow = row < kWRows ? qbase + row : t0 + (row - kWRows);
    const bool ok = row < kWRows ? grow < qend : grow < n_rows;
    const float* src = (row < kWRows ? qcoords : coords) + (size_t)grow * D;
#pragma unroll
    for (int k = 0; k < 4; ++k) st.t[k] = (ok && k0 + k < D) ? src[k0 + k] : 0.0f;
  }
}

__device__ __forceinline__ void stage_store(WideBuf& b, const Stage& st, bool last) {
#pragma unroll
  for (int m = 0; m < kWLoads; ++m) {
    const uint32_t e = threadIdx.x + kWBlock * m;   // (rows [32m, 32m + 32): query rows for m < 2)
    b.main[e >> 3][e & 7u] = m < kWRows / 32 ? st.v[m] : -st.v[m];
  }
  if (last && threadIdx.x < 2 * kWStage) b.tail[threadIdx.x >> 1][threadIdx.x & 1u] = st.t;
}

// one more column pair on two lane sums (DC_CANON_ACC, element-wise)
__device__ __forceinline__ f2 acc2(f2 a, f2 c) {
#ifdef DC_CANON_FMA
  return __builtin_elementwise_fma(c, c, a);
#else
  return a + c * c;
#endif
}

// the chunk in b onto the lane sums of this lane's pairs.  The reference rows are stored negated, so that the difference
// is one v_pk_add_f32 (LLVM splits a packed subtraction into two v_sub_f32); x + (-y) is x - y in IEEE arithmetic,
// NaN, infinities and the sign of zero included.
__device__ __forceinline__ void chunk_accumulate(const WideBuf& b, uint32_t qrow, uint32_t rrow,
                                                 f2 (&acc)[kTQ][kTR][kLanePairs]) {
#pragma unroll
  for (int kk = 0; kk < kWChunk / 4; ++kk) {
    constexpr int kHalves = kLanes / 4;
    const int h = 2 * (kk % kHalves);   // columns 4kk .. 4kk+3 -> lane sums 4(kk % kHalves) + 0..3
    f4 q[kTQ], r[kTR];
#pragma unroll
    for (int a = 0; a < kTQ; ++a) q[a] = b.main[qrow + 4 * a][kk];
#pragma unroll
    for (int c = 0; c < kTR; ++c) r[c] = b.main[kWRows + rrow + 16 * c][kk];
#pragma unroll
    for (int a = 0; a < kTQ; ++a)
#pragma unroll
      for (int c = 0; c < kTR; ++c) {
        acc[a][c][h] = acc2(acc[a][c][h], q[a].xy + r[c].xy);   // (q - r: r is stored negated)
        acc[a][c][h + 1] = acc2(acc[a][c][h + 1], q[a].zw + r[c].zw);
      }
  }
}

// the canonical d2 of one pair from its lane sums and the tail columns (rem = D - V of them): dist2_canon_rt /
// canon_sum_avx after their lane-sum loop, bit for bit
__device__ __forceinline__ float finish_pair(const f2 (&s)[kLanePairs], f4 qt0, f4 qt1, f4 rt0, f4 rt1, int rem) {
  const f4 c0 = qt0 - rt0, c1 = qt1 - rt1;
  auto col = [&](int k) { return k < 4 ? c0[k] : c1[k - 4]; };
#ifdef DC_CANON_AVX
  const f2 u = (s[0] + s[2]) + (s[1] + s[3]);   // (b0 + b2, b1 + b3) with b_i = a_i + a_{i+4}
  float d = u.x + u.y;
  if (rem >= 4) d = d + ((c0.x * c0.x + c0.z * c0.z) + (c0.y * c0.y + c0.w * c0.w));
  const int k4 = rem >= 4 ? 4 : 0;
#pragma unroll
  for (int k = 0; k < kWTail - 1; ++k)   // (constant k: no indexed register access)
    if (k >= k4 && k < rem) d = DC_CANON_ACC(d, col(k));
#else
  const f2 u = s[0] + s[1];   // (a0 + a2, a1 + a3)
  float d = u.x + u.y;
  if (rem >= 2) {
    d = d + (c0.x * c0.x + c0.y * c0.y);
    if (rem == 3) d = d + c0.z * c0.z;
  } else if (rem == 1) {
    d = d + c0.x * c0.x;
  }
  (void)col;
#endif
  return d;
}

// sum / lexicographic minimum over the 16 lanes of a wave that hold the same query rows (lane bits 2..5)
__device__ __forceinline__ uint32_t sum16(uint32_t v) {
#pragma unroll
  for (int off = 4; off < 64; off <<= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
  return v;
}
__device__ __forceinline__ unsigned long long min16(unsigned long long v) {
#pragma unroll
  for (int off = 4; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// pops (NR radius slots, kWidePop) / nearest neighbours (kWideNn) / pair list with pops (kWidePairs) / Boruvka min edge
// with pops (kWideMinEdge) of the query rows [i_from, i_to) against all n_rows rows
template <int MODE, int NR>
__global__ __launch_bounds__(kWBlock) void wide_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D,
                                                        uint32_t i_from, uint32_t i_to, WideArgs w,
                                                        const uint32_t* __restrict__ gate) {
  constexpr bool kCount = MODE != kWideNn;
  if (gate && gate[1] == 0) return;
  __shared__ WideBuf buf[2];
  __shared__ uint2 queues[MODE == kWidePairs ? (kWBlock / 64) * kPairQueue : 1];   // one pair queue per wave
  uint2* queue = queues + (MODE == kWidePairs ? (threadIdx.x >> 6) * kPairQueue : 0u);

  const uint32_t V = kLanes * (D / kLanes);
  const int rem = (int)(D - V);
  const uint32_t n_chunks = (V + kWChunk - 1) / kWChunk;   // (kMaxColsGeneric < D <= kMaxColsAny: 0 < V, no wrap)
  const uint32_t qbase = i_from + blockIdx.x * kWRows;
  const uint32_t qend = min(qbase + (uint32_t)kWRows, i_to);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tq = lane & 3u, tr = lane >> 2;
  const uint32_t qrow = 16u * wave + tq;   // this lane's query rows: qrow + 4a (block-relative)
  const uint32_t wave_lo = qbase + 16u * wave;

  uint32_t qi[kTQ];
  bool live[kTQ];
  float qfe[kTQ];
  uint32_t qc[kTQ], qr[kTQ];
#pragma unroll
  for (int a = 0; a < kTQ; ++a) {
    qi[a] = qbase + qrow + 4u * a;
    live[a] = qi[a] < qend;
    const uint32_t row = live[a] ? qi[a] : i_to - 1;   // clamp: result discarded
    qfe[a] = MODE != kWideNn ? 0.0f : !w.cross ? w.fe[row] : w.fe_q ? w.fe_q[row] : -INFINITY;
    qc[a] = MODE == kWideMinEdge ? w.g.comp[row] : 0u;
    qr[a] = MODE == kWideMinEdge ? w.g.rank[row] : 0u;
  }
  uint32_t cnt[kTQ][NR];
  unsigned long long best[kTQ], bhd[kTQ];   // nn: (d2 bits << 32 | j); min edge: the lightest key
#pragma unroll
  for (int a = 0; a < kTQ; ++a) {
#pragma unroll
    for (int r = 0; r < NR; ++r) cnt[a][r] = 0;
    best[a] = MODE == kWideNn ? ((unsigned long long)__float_as_uint(FLT_MAX) << 32) | (n_rows + 1u) : ~0ull;
    bhd[a] = best[a];
  }
  f2 acc[kTQ][kTR][kLanePairs];
#pragma unroll
  for (int a = 0; a < kTQ; ++a)
#pragma unroll
    for (int c = 0; c < kTR; ++c)
#pragma unroll
      for (int h = 0; h < kLanePairs; ++h) acc[a][c][h] = f2(0.0f);
  uint32_t fill = 0;

  Stage st;
  stage_load(coords, w.qcoords, n_rows, D, V, qend, qbase, 0u, 0u, n_chunks == 1, st);
  stage_store(buf[0], st, n_chunks == 1);
  __syncthreads();
  uint32_t t0 = 0, c = 0, cur = 0;   // tile, chunk of the tile, LDS buffer
  for (;;) {
    const bool last = c + 1 == n_chunks;
    const uint32_t nt0 = last ? t0 + kWRef : t0, nc = last ? 0u : c + 1;   // the next step
    const bool more = nt0 < n_rows;
    if (more) stage_load(coords, w.qcoords, n_rows, D, V, qend, qbase, nt0, nc * kWChunk, nc + 1 == n_chunks, st);
    const WideBuf& b = buf[cur];
    chunk_accumulate(b, qrow, tr, acc);
    if (last) {
      // finish the tile's pairs (reference rows t0 + tr + 16c) and hand them to the mode
      uint32_t rj[kTR];
      bool rok[kTR];
      float rfe[kTR];
      uint32_t rc[kTR], rr[kTR];
#pragma unroll
      for (int cc = 0; cc < kTR; ++cc) {
        rj[cc] = t0 + tr + 16u * cc;
        rok[cc] = rj[cc] < n_rows;
        const uint32_t j = rok[cc] ? rj[cc] : 0u;
        rfe[cc] = (MODE == kWideNn && w.fe) ? w.fe[j] : 0.0f;
        rc[cc] = MODE == kWideMinEdge ? w.g.comp[j] : 0u;
        rr[cc] = MODE == kWideMinEdge ? w.g.rank[j] : 0u;
      }
      const bool emit = t0 + kWRef > wave_lo + 1u;   // a pair is listed from its lower row
#pragma unroll
      for (int a = 0; a < kTQ; ++a) {
        const f4 qt0 = b.tail[qrow + 4 * a][0], qt1 = b.tail[qrow + 4 * a][1];
#pragma unroll
        for (int cc = 0; cc < kTR; ++cc) {
          const f4 rt0 = b.tail[kWRows + tr + 16 * cc][0], rt1 = b.tail[kWRows + tr + 16 * cc][1];
          const float d = finish_pair(acc[a][cc], qt0, qt1, rt0, rt1, rem);
          const uint32_t j = rj[cc];
          const bool ok = rok[cc] && (w.cross || j != qi[a]);
          if constexpr (kCount) {
#pragma unroll
            for (int r = 0; r < NR; ++r) cnt[a][r] += (ok && d < w.rad2.v[r]) ? 1u : 0u;
          }
          if constexpr (MODE == kWideNn) {
            // strict '<' in increasing j on this lane; lanes merge by the lexicographic (d2, j) minimum
            const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | j;
            const bool lt = ok && d < __uint_as_float((uint32_t)(best[a] >> 32));
            const bool lh = ok && rfe[cc] < qfe[a] && d < __uint_as_float((uint32_t)(bhd[a] >> 32));
            best[a] = lt ? key : best[a];
            bhd[a] = lh ? key : bhd[a];
          } else if constexpr (MODE == kWideMinEdge) {
            // (the self pair and every pair inside the component: same id)
            const unsigned long long key = ((unsigned long long)max(qr[a], rr[cc]) << 32) | min(qr[a], rr[cc]);
            best[a] = (ok && d < w.rad2.v[0] && rc[cc] != qc[a] && key < best[a]) ? key : best[a];
          } else if constexpr (MODE == kWidePairs) {
            if (emit) pair_push(ok && d < w.rad2.v[0] && live[a] && j > qi[a], qi[a], j, queue, fill, w.g);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < kTQ; ++a)
#pragma unroll
        for (int cc = 0; cc < kTR; ++cc)
#pragma unroll
          for (int h = 0; h < kLanePairs; ++h) acc[a][cc][h] = f2(0.0f);
    }
    if (!more) break;
    stage_store(buf[cur ^ 1u], st, nc + 1 == n_chunks);
    __syncthreads();
    t0 = nt0;
    c = nc;
    cur ^= 1u;
  }
  if constexpr (MODE == kWidePairs) {
    if (fill) pair_flush(queue, fill, w.g);
  }

  // merge the 16 lanes of each query row; lanes with tr == 0 write
#pragma unroll
  for (int a = 0; a < kTQ; ++a) {
    if constexpr (kCount) {
#pragma unroll
      for (int r = 0; r < NR; ++r) cnt[a][r] = sum16(cnt[a][r]);
    }
    if constexpr (MODE == kWideNn || MODE == kWideMinEdge) best[a] = min16(best[a]);
    if constexpr (MODE == kWideNn) bhd[a] = min16(bhd[a]);
    if (tr != 0 || !live[a]) continue;
    if constexpr (MODE == kWidePop) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < w.n_rad) w.g.pops[(size_t)r * (w.cross ? w.n_q : n_rows) + qi[a]] = cnt[a][r] + (w.cross ? 0u : 1u);
    } else if constexpr (MODE == kWideNn) {
      w.nn_idx[qi[a]] = (uint32_t)best[a];
      w.nn_d2[qi[a]] = __uint_as_float((uint32_t)(best[a] >> 32));
      if (!w.cross || w.fe_q) {
        w.hd_idx[qi[a]] = (uint32_t)bhd[a];
        w.hd_d2[qi[a]] = __uint_as_float((uint32_t)(bhd[a] >> 32));
      }
    } else {
      w.g.pops[qi[a]] = cnt[a][0] + 1u;
      if (MODE == kWideMinEdge && best[a] != ~0ull) atomicMin(w.g.best + qc[a], best[a]);
    }
  }
}

template <int MODE, int NR>
void wide_launch(const float* c, uint32_t n, uint32_t D, uint32_t i_from, uint32_t i_to, WideArgs w,
                 const uint32_t* gate, hipStream_t s) {
  if (i_to <= i_from) return;
  if (!w.cross) w.qcoords = c;
  const uint32_t grid = (i_to - i_from + kWRows - 1) / kWRows;
  hipLaunchKernelGGL((wide_kernel<MODE, NR>), dim3(grid), dim3(kWBlock), 0, s, c, n, D, i_from, i_to, w, gate);
}

}  // namespace

void launch_pop_wide(const float* d_coords, uint32_t n_rows, uint32_t n_cols, uint32_t i_from, uint32_t i_to,
                     const Rad2& rad2, int n_rad, uint32_t* d_pops, const uint32_t* gate, hipStream_t stream) {
  WideArgs w{};
  w.rad2 = rad2;
  w.n_rad = n_rad;
  w.g.pops = d_pops;
  // instances for 1, 4 and 8 radius slots; unused slots hold -1 ("d < -1" is never true)
  if (n_rad == 1)
    wide_launch<kWidePop, 1>(d_coords, n_rows, n_cols, i_from, i_to, w, gate, stream);
  else if (n_rad <= 4)
    wide_launch<kWidePop, 4>(d_coords, n_rows, n_cols, i_from, i_to, w, gate, stream);
  else
    wide_launch<kWidePop, 8>(d_coords, n_rows, n_cols, i_from, i_to, w, gate, stream);
}

void launch_nn_wide(const float* d_coords, uint32_t n_rows, uint32_t n_cols, const float* d_fe, uint32_t i_from,
                    uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2,
                    const uint32_t* gate, hipStream_t stream) {
  WideArgs w{};
  w.fe = d_fe;
  w.nn_idx = d_nn_idx;
  w.nn_d2 = d_nn_d2;
  w.hd_idx = d_hd_idx;
  w.hd_d2 = d_hd_d2;
  wide_launch<kWideNn, 1>(d_coords, n_rows, n_cols, i_from, i_to, w, gate, stream);
}

void launch_pop_cross_wide(const float* d_query, const float* d_ref, uint32_t n_q, uint32_t n_ref, uint32_t n_cols,
                           uint32_t i_from, uint32_t i_to, const Rad2& rad2, int n_rad, uint32_t* d_pops,
                           const uint32_t* gate, hipStream_t stream) {
  WideArgs w{};
  w.rad2 = rad2;
  w.n_rad = n_rad;
  w.g.pops = d_pops;
  w.qcoords = d_query;
  w.n_q = n_q;
  w.cross = 1;
  if (n_rad == 1)
    wide_launch<kWidePop, 1>(d_ref, n_ref, n_cols, i_from, i_to, w, gate, stream);
  else if (n_rad <= 4)
    wide_launch<kWidePop, 4>(d_ref, n_ref, n_cols, i_from, i_to, w, gate, stream);
  else
    wide_launch<kWidePop, 8>(d_ref, n_ref, n_cols, i_from, i_to, w, gate, stream);
}

void launch_nn_cross_wide(const float* d_query, const float* d_ref, uint32_t n_ref, uint32_t n_cols, const float* d_fe_q,
                          const float* d_fe_r, uint32_t i_from, uint32_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
                          uint32_t* d_hd_idx, float* d_hd_d2, const uint32_t* gate, hipStream_t stream) {
  WideArgs w{};
  w.fe = d_fe_q ? d_fe_r : nullptr;
  w.fe_q = d_fe_q;
  w.nn_idx = d_nn_idx;
  w.nn_d2 = d_nn_d2;
  w.hd_idx = d_hd_idx;
  w.hd_d2 = d_hd_d2;
  w.qcoords = d_query;
  w.cross = 1;
  wide_launch<kWideNn, 1>(d_ref, n_ref, n_cols, i_from, i_to, w, gate, stream);
}

void launch_pairs_wide(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2, uint32_t* d_pops,
                       uint2* d_pairs, unsigned long long capacity, unsigned long long* d_count, const uint32_t* gate,
                       hipStream_t stream) {
  WideArgs w{};
  w.rad2.v[0] = r2;
  w.n_rad = 1;
  w.g = GraphOut{d_pops, d_pairs, d_pairs ? capacity : 0ull, d_count, nullptr, nullptr, nullptr};
  wide_launch<kWidePairs, 1>(d_coords, n_rows, n_cols, 0, n_rows, w, gate, stream);
}

void launch_min_edge_wide(const float* d_coords, uint32_t n_rows, uint32_t n_cols, float r2, const uint32_t* d_comp,
                          const uint32_t* d_rank, uint32_t i_from, uint32_t i_to, unsigned long long* d_best,
                          uint32_t* d_pops, const uint32_t* gate, hipStream_t stream) {
  WideArgs w{};
  w.rad2.v[0] = r2;
  w.n_rad = 1;
  w.g = GraphOut{d_pops, nullptr, 0ull, nullptr, d_comp, d_rank, d_best};
  wide_launch<kWideMinEdge, 1>(d_coords, n_rows, n_cols, i_from, i_to, w, gate, stream);
}

}  // namespace dc
