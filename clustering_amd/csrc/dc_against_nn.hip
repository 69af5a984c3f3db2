// dc_against_nn.hip -- the pruned matrix-core neighbour sweep of new frames Q against a reference R
// (dc_hip_nearest_neighbors_cross_pruned_dev): nearest reference frame and nearest reference frame of strictly lower
// free energy.  Both sets are ordered by the cells of ONE grid on columns 0/1 (dc_prep.hpp against_key_kernel), R inside
// a cell by free energy; every 32-frame tile carries its box in that plane and R's tiles their free-energy range.  A
// wave visits R's tiles in rings of growing box distance from its query group and stops when the exact incumbents of
// all its queries lie inside the last ring: the ring logic of nn_pruned_kernel (dc_mfma_kernels.hpp), which is a
// statement about a query group and a set of tiles whichever arrays they come from.  What this kernel does not carry:
// the component view (one origin for both sets: a query may lie between the reference's clusters), the COOP form, the
// query's own position in the order (no reference row is the query), the seeds from the order (a query has no place in
// R's order) and the bounds published between shares before the final merge.  Built with the folded reference norms
// and the coarse early-out of nn_pruned_kernel: chains, thresholds, the wave-wide candidate queue and
// its canonical re-check are the helpers of dc_mfma_kernels.hpp.
#include "dc_mfma_kernels.hpp"
#include "dc_against_nn.hpp"

#ifndef DC_STEP_MASK
#define DC_STEP_MASK 0xFFFFu   // bit (n-1) set <=> the library is built for n MFMAs per tile pair
#endif

namespace dc {

namespace {

// merge of several reference shares, by query POSITION: words (d2 bits << 32 | reference row), "none" to start with
__global__ void nn_against_fill_kernel(unsigned long long* __restrict__ merge64, uint32_t n_words, uint32_t n_ref) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_words) merge64[i] = ((unsigned long long)__float_as_uint(FLT_MAX) << 32) | (n_ref + 1);
}
__global__ void nn_against_unpack_kernel(const unsigned long long* __restrict__ merge64,
                                         const uint32_t* __restrict__ perm_q, uint32_t n_pos,
                                         const uint32_t* __restrict__ hdr, uint32_t* __restrict__ nn_idx,
                                         float* __restrict__ nn_d2, uint32_t* __restrict__ hd_idx,
                                         float* __restrict__ hd_d2) {
  if (hdr[1] != 0) return;   // flagged data: the sweep stood down, the gated direct kernel writes
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pos) return;
  const uint32_t i = perm_q[p];
  if (i == kInvalidFrame) return;   // (a pad position of the order)
  const unsigned long long a = merge64[p], b = merge64[(size_t)n_pos + p];
  nn_idx[i] = (uint32_t)a;
  nn_d2[i] = __uint_as_float((uint32_t)(a >> 32));
  if (hd_idx) {
    hd_idx[i] = (uint32_t)b;
    hd_d2[i] = __uint_as_float((uint32_t)(b >> 32));
  }
}

// One wave owns TQ consecutive query tiles of Q's order and one share (blockIdx.y of gridDim.y, round-robin) of R's
// tiles.  Results by query row: written when there is one share, merged into A.merge64 otherwise.
template <int NM, int TQ>
__global__ __launch_bounds__(256, 2) void nn_against_kernel(NnAgainstArgs A, uint32_t n_cols,
                                                            uint32_t* __restrict__ nn_idx, float* __restrict__ nn_d2,
                                                            uint32_t* __restrict__ hd_idx, float* __restrict__ hd_d2) {
  // dynamic LDS, per wave: the survivor list of a scan round [kListCap], the candidate list [kWaveQueue] x 8 B and the
  // packed exact incumbents [2][TQ * 32] x 8 B; behind them the query rows [TQ * 32][n_cols] (original coordinates)
  extern __shared__ __attribute__((aligned(16))) float nn_against_lds[];
  static_assert(TQ % 2 == 0 && TQ * 32 <= 256, "accumulator ping-pong; query index of a queue entry");
  uint32_t* __restrict__ hdr = A.hdr;
  if (hdr[1] != 0) return;   // flagged data: the gated direct kernel runs instead
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) hdr[kHdrShares] = gridDim.y;
  const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int wib = threadIdx.x >> 6;
  const uint32_t wpb = blockDim.x >> 6;
  const uint32_t TQT = A.T_q, T = A.T_r, n_ref = A.n_ref;
  const uint32_t n_groups = (TQT + TQ - 1) / TQ;
  const uint32_t blk_unit = xcd_block((n_groups + wpb - 1) / wpb);
  if (blk_unit == 0xFFFFFFFFu) return;   // (pad block of the grid)
  const uint32_t wave = blk_unit * wpb + wib;
  const uint32_t chunk = blockIdx.y, n_chunks = gridDim.y;
  const uint32_t qt0 = wave * TQ;
  if (qt0 >= TQT) return;    // whole wave leaves; no block-level barriers in this kernel
  constexpr uint32_t kWaveWords = kListCap + 2 * kWaveQueue + 4 * TQ * 32;
  uint32_t* list = reinterpret_cast<uint32_t*>(nn_against_lds) + (size_t)wib * kWaveWords;
  uint2* cand = reinterpret_cast<uint2*>(list + kListCap);
  unsigned long long* best64 = reinterpret_cast<unsigned long long*>(list + kListCap + 2 * kWaveQueue);
  float* qrows = nn_against_lds + (size_t)wpb * kWaveWords + (size_t)wib * (TQ * 32) * n_cols;
  uint32_t qn = 0;   // queued candidates (wave-uniform)

  // (scaled units, like the accumulators and the running minima taken from them)
  const Scale sc = load_scale(hdr);   // (the neighbour scale: scale_kernel ran before the images were built)
  const GuardBand gb = guard_band(__uint_as_float(hdr[kHdrMused]) * sc.s2, 0.0f, (int)n_cols, sc, true);   // (folded norms)
  // (the cached thresholds q[].bn / q[].bh INCLUDE the skip bound of the early-out, as in nn_pruned_kernel)
  const float skipb = kNnEarly<NM> ? nn_skip_bound(__uint_as_float(hdr[kHdrMused]) * sc.s2) : 0.0f;
  const bool have_fe = A.fe_q != nullptr;

  s16x8 b[TQ][NM];
  NnPQr q[TQ];   // (m_nn, m_hd in d2 units; bn, bh in the accumulators' units: c_q taken off)
  float cq[TQ];  // |x'|^2 of the lane's query (scaled units)
  uint32_t jq[TQ];
  uint64_t livemask[TQ];
  float4 gbox = make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);
#pragma unroll
  for (int qt = 0; qt < TQ; ++qt) {
    const uint32_t tile = qt0 + qt;
    const uint32_t tl = tile < TQT ? tile : TQT - 1;
    const uint32_t frame = (tile < TQT) ? A.perm_q[tile * 32 + c] : kInvalidFrame;
    const bool live = frame != kInvalidFrame;
    livemask[qt] = __builtin_amdgcn_ballot_w64(live);
    jq[qt] = live ? frame : 0u;
    load_query_folded<NM>(A.img_q, tl, lane, h, live, sc, b[qt]);
    cq[qt] = live ? A.norms_q[tl * 32 + c] : 0.0f;
    // a NaN free energy has no lower frame, like -inf (tested on the bits: this unit is compiled without NaN semantics)
    float f = (live && have_fe) ? A.fe_q[jq[qt]] : -INFINITY;
    if ((__float_as_uint(f) & 0x7FFFFFFFu) > 0x7F800000u) f = -INFINITY;
    q[qt].feq = f;
    q[qt].spos = 0xFFFFFFFFu;   // (no reference row is the query itself)
    q[qt].m_nn = live ? INFINITY : -INFINITY;   // idle lanes can never trigger the exact path
    q[qt].m_hd = live ? INFINITY : -INFINITY;
    q[qt].bn = nn_prime(nn_band(gb, q[qt].m_nn), cq[qt]) + skipb;
    q[qt].bh = nn_prime(nn_band(gb, q[qt].m_hd), cq[qt]) + skipb;
    const float4 qb = (tile < TQT) ? A.box_q[tile] : make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);
    gbox.x = fminf(gbox.x, qb.x);
    gbox.y = fmaxf(gbox.y, qb.y);
    gbox.z = fminf(gbox.z, qb.z);
    gbox.w = fmaxf(gbox.w, qb.w);
  }
#pragma unroll
  for (int qt = 0; qt < TQ; ++qt) {
    stage_query_rows(qrows + (size_t)qt * 32 * n_cols, nullptr, A.qcoords, jq[qt], (livemask[qt] >> lane) & 1, n_cols, lane);
    // the exact incumbents of the wave's queries live in LDS as order-preserving words (see nn_wave_flush)
    if (h == 0) {
      best64[qt * 32 + c] = ((unsigned long long)__float_as_uint(FLT_MAX) << 32) | (n_ref + 1);
      best64[TQ * 32 + qt * 32 + c] = ((unsigned long long)__float_as_uint(FLT_MAX) << 32) | (n_ref + 1);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // (query rows and incumbents: written by the h = 0 lanes)
  // lowest free energy of the reference (header word 12, ordered-integer key, written by the pass over fe_ref): a
  // query at or below that level has no lower frame -- nn_hd is closed for it from the start
  const float fe_floor = have_fe ? fkey_inv(~hdr[12]) : INFINITY;
  // evaluate and empty the candidate list (64 candidates at a time, one per lane)
  auto flush = [&]() {
    nn_wave_flush(cand, qn, qrows, best64, TQ * 32, A.coords_r, A.perm_r, n_cols, lane);
    qn = 0;
  };
  uint32_t chains = 0, visited = 0;
  uint32_t chains_on = 0;   // chains that went on behind the early-out test (computed again in full)
  // this wave's share of the reference tiles: t = chunk + u * n_chunks, u = 0 .. U-1
  const uint32_t U = (T > chunk) ? (T - chunk + n_chunks - 1) / n_chunks : 0u;
  auto tile_of = [&](uint32_t u) { return chunk + u * n_chunks; };
  // rings: r2_lo <= gap2 < r2_hi.  The first one covers the group's own extent, a cell of the grid, and the way to the
  // reference's bounding box: a group far outside R would otherwise scan its share about twenty times (x 4 per empty
  // ring) before it meets a tile
  const float dgx = gbox.y - gbox.x, dgy = gbox.w - gbox.z;
  const float gap_r = box_gap2(gbox, make_float4(A.meta[0], A.meta[1], A.meta[2], A.meta[3]));
  float r2_lo = -1.0f;
  float r2_hi = fmaxf(fmaxf(dgx * dgx + dgy * dgy, A.meta[4]), gap_r * 1.001f);
  if (!(r2_hi > 0.0f)) r2_hi = FLT_MIN;
  if (!(r2_hi < 1.0e37f)) r2_hi = INFINITY;
  for (;;) {
    for (uint32_t base = 0; base < U; base += kListCap) {
      // ---- scan: which reference tiles of this round lie in the ring?
      uint32_t cnt = 0;
      const uint32_t lim = min(U - base, (uint32_t)kListCap);
      float4 rb_next = ((uint32_t)lane < lim) ? A.box_r[tile_of(base + lane)]
                                              : make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);
      for (uint32_t k = 0; k < lim; k += 64) {
        const uint32_t t = tile_of(base + k + lane);
        const float4 rb = rb_next;   // fetched one step ahead: the scan is latency-bound otherwise
        if (k + 64 + lane < lim) rb_next = A.box_r[tile_of(base + k + 64 + lane)];
        bool ok = false;
        if (k + lane < lim) {
          const float g2 = box_gap2(gbox, rb);
          ok = (g2 < r2_hi) & (g2 >= r2_lo);
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(ok);
        if (ok) list[cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0))] = t;
        cnt += (uint32_t)__builtin_popcountll(m);
      }
      if (cnt == 0) continue;
      visited += cnt;
      s16x8 a0[NM];
      auto entry = [&](uint32_t i) {
        return (uint32_t)__builtin_amdgcn_readfirstlane(list[i < cnt ? i : cnt - 1]);
      };
      // the rest of an epilogue: free-energy classes, band test, parking of the candidates (nn_pruned_kernel's, without
      // the query's own position).  (t, fr) describe the reference tile the accumulator belongs to.
      auto finish = [&](const f32x16& acc, auto qi_c, float tmin, uint32_t t, float2 fr) __attribute__((always_inline)) {
        constexpr int qi = decltype(qi_c)::value;
        NnPQr& Q = q[qi];
        // (bh >= bn always, so a tile that has lower frames is tested against bh alone, any other against bn)
        const float thr = (fr.x < Q.feq) ? Q.bh : Q.bn;
        const bool rare = tmin < thr;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(rare) != 0, 0)) {
          // the free-energy mask: a tile entirely lower gives the hd minimum from the nn minimum, a tile entirely not
          // lower contributes nothing to hd, a mixed tile takes the per-element minima
          const bool all_lower = fr.y < Q.feq;
          const bool mixed = (fr.x < Q.feq) & !all_lower;
          float hmin = all_lower ? tmin : INFINITY;
          const bool any_mixed = __builtin_amdgcn_ballot_w64(mixed) != 0;
          if (any_mixed) {
            const NnMin g = nn_special_fe(acc, A.fe_c, t, h, Q.spos, Q.feq);   // valid for every lane, just slower
            tmin = g.tmin;
            hmin = g.hmin;
          }
          // (the two half-wave lanes of a query see different rows of every tile: the running minima are shared)
          float new_nn = fminf(Q.m_nn, nn_unprime(tmin, cq[qi])), new_hd = fminf(Q.m_hd, nn_unprime(hmin, cq[qi]));
          new_nn = fminf(new_nn, __shfl_xor(new_nn, 32, 64));
          new_hd = fminf(new_hd, __shfl_xor(new_hd, 32, 64));
          const float bn = nn_prime(nn_band(gb, new_nn), cq[qi]), bh = nn_prime(nn_band(gb, new_hd), cq[qi]);
          const bool trig = (tmin < bn) | (hmin < bh);
          if (__builtin_amdgcn_ballot_w64(trig) != 0) {
            // park this tile's candidates (values within the band of the running minima); element r of the accumulator
            // is bit (15 - r) of the masks
            uint32_t mn = 0, mh = 0;
            if (!any_mixed && t + 1 != T) {
              // plain tile: below-threshold sign strings (idle lanes have thresholds of -inf, pad rows only exist in
              // the last tile)
              uint32_t sn = 0, sh = 0;
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                sn = __builtin_amdgcn_alignbit(sn, __float_as_uint(acc[r] - bn), 31);
                sh = __builtin_amdgcn_alignbit(sh, __float_as_uint(acc[r] - bh), 31);
              }
              mn = sn & 0xFFFFu;
              mh = all_lower ? (sh & 0xFFFFu) : 0u;
            } else {
              float4 fv[4];
              load_frag(A.fe_c, t, h, fv);
              const f32x16 fef = frag16(fv);
              const bool live = (livemask[qi] >> lane) & 1;
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                mn |= (live & (acc[r] < bn)) ? (0x8000u >> r) : 0u;
                mh |= (live & (acc[r] < bh) & (fef[r] < Q.feq)) ? (0x8000u >> r) : 0u;
              }
            }
            uint32_t m = mn | mh;
            for (;;) {
              const uint64_t have = __builtin_amdgcn_ballot_w64(m != 0);
              if (have == 0) break;
              const uint32_t n_new = (uint32_t)__builtin_popcountll(have);
              if (qn + n_new > (uint32_t)kWaveQueue) flush();
              if (m != 0) {
                const int p = __builtin_ctz(m);
                const uint32_t slot = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(have >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)have, 0));
                cand[slot] = make_uint2(tile_row(t, 15 - p, h) | (((mn >> p) & 1u) << 30) | (((mh >> p) & 1u) << 31),
                                        (uint32_t)(qi * 32 + c));
                m &= m - 1;
              }
              qn += n_new;
            }
            if (qn >= 64u) flush();
          }
          Q.m_nn = new_nn;
          Q.m_hd = new_hd;
          Q.bn = bn + skipb;
          Q.bh = bh + skipb;
        }
      };
      // Full chains (NM = 1 and the single-buffer instances): accB always holds the chain whose epilogue is still
      // pending.  The early-out form (kNnEarly) keeps nothing pending across tiles and uses accA / accB as its two coarse
      // accumulators.
      f32x16 accA, accB;
#pragma unroll
      for (int r = 0; r < 16; ++r) accB[r] = INFINITY;
      uint32_t tB = 0;
      float2 frB = make_float2(INFINITY, INFINITY);
      auto compute = [&](s16x8 (&a)[NM], uint32_t t, uint32_t t_next, float2 fr) {
        f32x16 c0;
#pragma unroll
        for (int r = 0; r < 16; ++r) c0[r] = 0.0f;   // (an inline constant of the first MFMA)
        chains += TQ;
        if constexpr (kNnEarly<NM>) {
          // the coarse minima of the tile's TQ chains are tested together; a chain that goes on is computed again from
          // its first MFMA (nn_pruned_kernel)
          float tm[TQ], dmin = INFINITY;
          accA = mfma16(a[0], b[0][0], c0);
#pragma unroll
          for (int m = 1; m < kNnCoarse<NM>; ++m) accA = mfma16(a[m], b[0][m], accA);
          constexpr_for_pairs<TQ>([&](auto qt_c) {
            constexpr int qt = decltype(qt_c)::value;
            tm[qt] = INFINITY;
            nn_chain_coarse<NM, kNnCoarse<NM>, NM>(a, b[qt + 1], c0, accB, accA, tm[qt]);
            tm[qt + 1] = INFINITY;
            if constexpr (qt + 2 < TQ)
              nn_chain_coarse<NM, kNnCoarse<NM>, NM>(a, b[qt + 2], c0, accA, accB, tm[qt + 1]);
            else
              tile_min<0, 16>(accB, tm[qt + 1]);
          });
#pragma unroll
          for (int qi = 0; qi < TQ; ++qi) dmin = fminf(dmin, tm[qi] - ((fr.x < q[qi].feq) ? q[qi].bh : q[qi].bn));
          if (__builtin_expect(__builtin_amdgcn_ballot_w64(dmin < 0.0f) != 0, 0)) {
            constexpr_for_all<TQ>([&](auto qi_c) {
              constexpr int qi = decltype(qi_c)::value;
              const float thr_c = (fr.x < q[qi].feq) ? q[qi].bh : q[qi].bn;
              if (__builtin_amdgcn_ballot_w64(tm[qi] < thr_c) != 0) {
                chains_on += 1;
                f32x16 acc = mfma16(a[0], b[qi][0], c0);
#pragma unroll
                for (int m = 1; m < NM; ++m) acc = mfma16(a[m], b[qi][m], acc);
                float tmin = INFINITY;
                tile_min<0, 16>(acc, tmin);
                finish(acc, qi_c, tmin, t, fr);
              }
            });
          }
          return;
        }
        auto refill = [&](auto mi_c) {
          if constexpr (kSingleBuffer<NM>) {
            constexpr int MI = decltype(mi_c)::value;
            const uint4 v = A.img_r[(size_t)t_next * (NM * 64) + MI * 64 + lane];
            a[MI] = __builtin_bit_cast(s16x8, v);
          }
        };
        constexpr_for_pairs<TQ>([&](auto qt_c) {
          constexpr int qt = decltype(qt_c)::value;
          constexpr int qb = (qt == 0) ? TQ - 1 : qt - 1;
          float tmin = INFINITY;
          nn_chain<NM>(a, b[qt], c0, accA, accB, tmin);
          finish(accB, std::integral_constant<int, qb>{}, tmin, (qt == 0) ? tB : t, (qt == 0) ? frB : fr);
          tmin = INFINITY;
          if constexpr (qt + 2 == TQ)   // last chain of the tile
            nn_chain<NM>(a, b[qt + 1], c0, accB, accA, tmin, refill);
          else
            nn_chain<NM>(a, b[qt + 1], c0, accB, accA, tmin);
          finish(accA, std::integral_constant<int, qt>{}, tmin, t, fr);
        });
        tB = t;
        frB = fr;
      };
      if constexpr (kSingleBuffer<NM>) {
        uint32_t t0 = entry(0);
        load_tile_folded<NM>(A.img_r, t0, lane, a0);
        float2 f0 = A.ferange_r[t0];
        for (uint32_t i = 0; i < cnt; ++i) {
          const uint32_t t1 = entry(i + 1);
          const float2 f1 = A.ferange_r[t1];
          compute(a0, t0, t1, f0);
          t0 = t1;
          f0 = f1;
        }
      } else {
        s16x8 a1[NM];
        // (the survivor list is read one tile ahead of its use)
        auto peek = [&](uint32_t i) { return list[i < cnt ? i : cnt - 1]; };
        uint32_t t0 = entry(0), t1;
        uint32_t l_next = peek(1);
        load_tile_folded<NM>(A.img_r, t0, lane, a0);
        float2 f0 = A.ferange_r[t0], f1;
        for (uint32_t i = 0; i < cnt; i += 2) {
          t1 = (uint32_t)__builtin_amdgcn_readfirstlane(l_next);
          l_next = peek(i + 2);
          load_tile_folded<NM>(A.img_r, t1, lane, a1);
          f1 = A.ferange_r[t1];
          compute(a0, t0, t1, f0);
          if (i + 1 < cnt) {
            t0 = (uint32_t)__builtin_amdgcn_readfirstlane(l_next);
            l_next = peek(i + 3);
            load_tile_folded<NM>(A.img_r, t0, lane, a0);
            f0 = A.ferange_r[t0];
            compute(a1, t1, t0, f1);
          }
        }
      }
      if constexpr (!kNnEarly<NM>) {  // drain: epilogue of the last pending chain of this round
        float tmin = INFINITY;
        tile_min<0, 16>(accB, tmin);
        finish(accB, std::integral_constant<int, TQ - 1>{}, tmin, tB, frB);
      }
    }
    flush();                                          // the settle test needs the exact incumbents (in LDS)
    if (!(r2_hi <= FLT_MAX) || visited >= U)
      break;   // every reference tile of this wave's share has been visited
    // settled: every unvisited frame is >= sqrt(r2_hi) away; the exact incumbents decide.  The margin and the strict
    // '<' keep ties on the lowest index: a frame at exactly the incumbent's distance may sit in a tile whose box gap
    // equals that distance, i.e. in the NEXT ring.
    const float sure = r2_hi * 0.9999f;
    // The next ring must cover the WORST open query of the group: the largest incumbent still to be confirmed.
    float need = 0.0f;
#pragma unroll
    for (int qt = 0; qt < TQ; ++qt) {
      const bool live = (livemask[qt] >> lane) & 1;
      const bool hd_possible = fe_floor < q[qt].feq;
      // (both half-wave lanes of a query read the same words)
      const float inc_nn = __uint_as_float((uint32_t)(best64[qt * 32 + c] >> 32));
      const float inc_hd = __uint_as_float((uint32_t)(best64[TQ * 32 + qt * 32 + c] >> 32));
      const float want = fminf(fmaxf(inc_nn, hd_possible ? inc_hd : 0.0f), 3.0e38f);   // (no candidate at all: 3e38)
      const bool open = live & (h == 0) & !(want < sure);
      need = fmaxf(need, open ? want : 0.0f);
    }
    need = wave_max(need);
    if (!(need > 0.0f)) break;   // every query of the group is settled
    r2_lo = r2_hi;
    if (need >= 1.0e38f)
      r2_hi = r2_hi * 4.0f;   // (a query without any candidate yet)
    else
      r2_hi = fmaxf(need * 1.001f, r2_hi * 1.001f);
    if (!(r2_hi < 1.0e37f)) r2_hi = INFINITY;
  }
  if (lane == 0 && chains != 0u) {
    unsigned long long* chain_counter = reinterpret_cast<unsigned long long*>(hdr + 4);
    atomicAdd(chain_counter, (unsigned long long)chains);
    atomicAdd(chain_counter + kMfmaCtrNn, kNnEarly<NM> ? (unsigned long long)chains * kNnCoarse<NM> + (unsigned long long)chains_on * NM
                                                       : (unsigned long long)chains * NM);
  }

  const uint32_t n_pos = 32u * TQT;
#pragma unroll
  for (int qt = 0; qt < TQ; ++qt) {
    if (h == 0 && ((livemask[qt] >> lane) & 1)) {
      const unsigned long long w_nn = best64[qt * 32 + c], w_hd = best64[TQ * 32 + qt * 32 + c];
      if (n_chunks == 1) {
        nn_idx[jq[qt]] = (uint32_t)w_nn;
        nn_d2[jq[qt]] = __uint_as_float((uint32_t)(w_nn >> 32));
        if (hd_idx) {
          hd_idx[jq[qt]] = (uint32_t)w_hd;
          hd_d2[jq[qt]] = __uint_as_float((uint32_t)(w_hd >> 32));
        }
      } else {
        // d2 >= 0, so (d2 bits << 32 | reference row) orders like the lexicographic (d2, row): the merge over the shares
        // is a 64-bit atomic min (merge64 was filled with (FLT_MAX, n_ref + 1))
        const uint32_t pos = (qt0 + qt) * 32 + c;
        atomicMin(&A.merge64[pos], w_nn);
        atomicMin(&A.merge64[(size_t)n_pos + pos], w_hd);
      }
    }
  }
}

template <int S>
void nn_against_dispatch(const NnAgainstArgs& A, uint32_t n_cols, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx,
                         float* hd_d2, hipStream_t s) {
  constexpr int TQ = tq_nn(S);
  const uint32_t waves = (A.T_q + TQ - 1) / TQ;
  if (waves == 0 || A.T_r == 0) return;
  const uint32_t wpb = waves_per_group(S, sweep_switches());
  const uint32_t n_chunks = pick_chunks(waves * TQ, TQ, kNnWaveTargetPerWave, A.T_r, kNnShareFloor, (size_t)S * 1024 + 128);
  const dim3 grid(grid_x8((waves + wpb - 1) / wpb), n_chunks), block(64 * wpb);
  const size_t smem = wpb * (sizeof(uint32_t) * (kListCap + 2 * kWaveQueue + 4 * TQ * 32) + sizeof(float) * TQ * 32 * (size_t)n_cols);
  if (smem > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nn_against_kernel<S, TQ>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const uint32_t n_pos = 32u * A.T_q;
  if (n_chunks > 1)
    hipLaunchKernelGGL(nn_against_fill_kernel, dim3((2 * n_pos + 255) / 256), dim3(256), 0, s, A.merge64, 2 * n_pos, A.n_ref);
  timed_launch(1, s, [&] {
    hipLaunchKernelGGL((nn_against_kernel<S, TQ>), grid, block, smem, s, A, n_cols, nn_idx, nn_d2, hd_idx, hd_d2);
  });
  if (n_chunks > 1)
    hipLaunchKernelGGL(nn_against_unpack_kernel, dim3((n_pos + 255) / 256), dim3(256), 0, s,
                       (const unsigned long long*)A.merge64, A.perm_q, n_pos, (const uint32_t*)A.hdr, nn_idx, nn_d2, hd_idx,
                       hd_d2);
}

// (only the instances of the MFMA counts the library is built for -- DC_STEP_MASK, as in dc_mfma.hip -- exist)
template <int S>
void nn_against_step(const NnAgainstArgs& A, uint32_t n_cols, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx,
                     float* hd_d2, hipStream_t s) {
  if constexpr (((DC_STEP_MASK >> (S - 1)) & 1u) != 0) nn_against_dispatch<S>(A, n_cols, nn_idx, nn_d2, hd_idx, hd_d2, s);
}

}  // namespace

#define DC_FOR_EACH_S(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13)

void nn_against_sweep(const NnAgainstArgs& A, uint32_t n_cols, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx,
                      float* hd_d2, hipStream_t s) {
  switch (nm_for((int)n_cols)) {
#define X_(SV)                                                        \
  case SV:                                                            \
    nn_against_step<SV>(A, n_cols, nn_idx, nn_d2, hd_idx, hd_d2, s);  \
    break;
    DC_FOR_EACH_S(X_)
#undef X_
    default:
      break;
  }
}

}  // namespace dc
