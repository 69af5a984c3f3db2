// dc_against.hip -- the pruned matrix-core population sweep of new frames Q against a reference R
// (DC_VARIANT_CROSS_PRUNED).  Both sets are ordered by the cells of ONE grid on columns 0/1 (dc_prep.hpp
// against_key_kernel), every 32-frame tile of either order carries its box in that plane, and a (query group,
// reference tile) pair whose boxes are at least r_max apart is never touched -- the rule of pop_pruned_kernel, which
// is a statement about two tiles whichever arrays they come from.  What this kernel does not carry: the symmetric
// form and the self-term correction (a rectangle has neither), the pair sinks, and the component view (one origin
// for both sets: a query may lie between the reference's clusters).  Chains, folded threshold, two-bit epilogue,
// the wave-wide queue of band pairs and their canonical re-check are the helpers of dc_mfma_kernels.hpp.
#include "dc_mfma_kernels.hpp"
#include "dc_against.hpp"

#ifndef DC_STEP_MASK
#define DC_STEP_MASK 0xFFFFu   // bit (n-1) set <=> the library is built for n MFMAs per tile pair
#endif

namespace dc {

namespace {

// One wave owns TQ consecutive query tiles of Q's order and one share (blockIdx.y of gridDim.y, round-robin) of R's
// tiles.  One radius per launch: rad2.v[0].  pops: by query row, written when there is one share, added otherwise.
template <int NM, int TQ>
__global__ __launch_bounds__(256, 2) void pop_against_kernel(AgainstArgs A, uint32_t n_cols, Rad2 rad2,
                                                             uint32_t* __restrict__ pops) {
  // dynamic LDS, per wave: the survivor list of a scan round [kListCap], the query rows [TQ * 32][n_cols] (original
  // coordinates), the wave's queue of band pairs [kWaveQueue] and the counts the exact path found [TQ * 32]
  extern __shared__ __attribute__((aligned(16))) float against_lds[];
  static_assert(TQ % 2 == 0 && TQ * 32 <= 256, "accumulator ping-pong; the queue entry holds the query in 8 bits");
  const uint32_t* __restrict__ hdr = A.hdr;
  if (hdr[1] != 0) return;   // flagged data: the gated direct kernel runs instead
  const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int wib = threadIdx.x >> 6;
  const uint32_t wpb = blockDim.x >> 6;
  const uint32_t TQT = A.T_q, T = A.T_r;
  const uint32_t n_groups = (TQT + TQ - 1) / TQ;
  const uint32_t blk_unit = xcd_block((n_groups + wpb - 1) / wpb);
  if (blk_unit == 0xFFFFFFFFu) return;   // (pad block of the grid)
  const uint32_t wave = blk_unit * wpb + wib;
  const uint32_t chunk = blockIdx.y, n_chunks = gridDim.y;
  const uint32_t qt0 = wave * TQ;
  if (qt0 >= TQT) return;    // whole wave leaves; no block-level barriers in this kernel
  constexpr uint32_t kWaveWords = kListCap + kWaveQueue + TQ * 32;
  uint32_t* list = reinterpret_cast<uint32_t*>(against_lds) + (size_t)wib * kWaveWords;
  uint32_t* queue = list + kListCap;
  uint32_t* fix_tab = queue + kWaveQueue;
  float* qrows = against_lds + (size_t)wpb * kWaveWords + (size_t)wib * (TQ * 32) * n_cols;
  uint32_t qn = 0;   // queued band pairs (wave-uniform)

  const PopSetup<1> P = pop_setup<1>(hdr, rad2, n_cols);
  const float r2 = rad2.v[0];
  const float far2 = r2 * 1.0001f;   // boxes at least this far apart (squared) hold no pair inside

  s16x8 b[TQ][NM];
  uint32_t cnt_q[TQ], jq[TQ];
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
    const float cq = live ? A.norms_q[tl * 32 + c] - P.rad2e.v[0] : dead_const(P.sc);
    load_query<NM>(A.img_q, tl, lane, h, cq, P.sc, b[qt]);
    cnt_q[qt] = 0;
    const float4 qb = (tile < TQT) ? A.box_q[tile] : make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);
    gbox.x = fminf(gbox.x, qb.x);
    gbox.y = fmaxf(gbox.y, qb.y);
    gbox.z = fminf(gbox.z, qb.z);
    gbox.w = fmaxf(gbox.w, qb.w);
  }
#pragma unroll
  for (int qt = 0; qt < TQ; ++qt) {
    stage_query_rows(qrows + (size_t)qt * 32 * n_cols, nullptr, A.qcoords, jq[qt], (livemask[qt] >> lane) & 1, n_cols, lane);
    if (h == 0) fix_tab[qt * 32 + c] = 0;
  }

  auto flush_wave = [&]() {
    pop_wave_flush_rows(queue, qn, qrows, fix_tab, A.coords_r, n_cols, r2, lane);
    qn = 0;
  };

  uint32_t chains = 0;
  // this wave's share of the reference tiles: t = chunk + u * n_chunks, u = 0 .. U-1
  const uint32_t U = (T > chunk) ? (T - chunk + n_chunks - 1) / n_chunks : 0u;
  for (uint32_t base = 0; base < U; base += kListCap) {
    // ---- scan: which reference tiles of this round can hold a pair within r_max of the group?
    uint32_t cnt = 0;
    const uint32_t lim = min(U - base, (uint32_t)kListCap);
    auto tile_of = [&](uint32_t u) { return chunk + u * n_chunks; };
    float4 rb_next = ((uint32_t)lane < lim) ? A.box_r[tile_of(base + lane)]
                                            : make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);
    for (uint32_t k = 0; k < lim; k += 64) {
      const uint32_t t = tile_of(base + k + lane);
      const float4 rb = rb_next;
      if (k + 64 + lane < lim) rb_next = A.box_r[tile_of(base + k + 64 + lane)];
      const bool ok = (k + lane < lim) && (box_gap2(gbox, rb) < far2);
      const uint64_t m = __builtin_amdgcn_ballot_w64(ok);
      if (ok) list[cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0))] = t;
      cnt += (uint32_t)__builtin_popcountll(m);
    }
    if (cnt == 0) continue;
    // ---- the survivors: chains software-pipelined over two accumulator tiles (pop_pruned_kernel)
    s16x8 a0[NM];
    float4 n0[4];
    auto entry = [&](uint32_t i) {
      return (uint32_t)__builtin_amdgcn_readfirstlane(list[i < cnt ? i : cnt - 1]);
    };
    // the rest of an epilogue: counts, band test, parking of the band pairs.  Pad rows (acc = +inf) and idle lanes
    // (dead_const) are never in a band.
    auto finish = [&](auto qi_c, const PopAcc<1>& e, uint32_t t) {
      constexpr int qi = decltype(qi_c)::value;
      cnt_q[qi] += __builtin_popcount(inside_of(e.bits[0]));
      uint32_t m = band_of(e.bits[0]);
      if (__builtin_expect((__builtin_amdgcn_ballot_w64(m != 0) & livemask[qi]) != 0, 0)) {
        for (;;) {
          const uint64_t have = __builtin_amdgcn_ballot_w64(m != 0);
          if (have == 0) break;
          const uint32_t n_new = (uint32_t)__builtin_popcountll(have);
          if (qn + n_new > (uint32_t)kWaveQueue) flush_wave();
          if (m != 0) {
            const int p = __builtin_ctz(m);
            const uint32_t slot = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(have >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)have, 0));
            queue[slot] = tile_row(t, element_of(p), h) | ((uint32_t)(qi * 32 + c) << kPopQueuePosBits);
            m &= m - 1;
          }
          qn += n_new;
        }
        if (qn >= 64u) flush_wave();
      }
    };
    f32x16 accA, accB;   // accB: the chain whose epilogue is pending (+inf everywhere = contributes nothing)
#pragma unroll
    for (int r = 0; r < 16; ++r) accB[r] = INFINITY;
    uint32_t tB = 0;
    auto compute = [&](s16x8 (&a)[NM], float4 (&nv)[4], uint32_t t, uint32_t t_next) {
      const f32x16 c0 = frag16(nv);
      chains += TQ;
      auto refill = [&](auto mi_c) {
        if constexpr (kSingleBuffer<NM>)
          refill_frag<NM, decltype(mi_c)::value>(A.img_r, A.norms_r, t_next, lane, h, a, nv);
      };
      constexpr_for_pairs<TQ>([&](auto qt_c) {
        constexpr int qt = decltype(qt_c)::value;
        constexpr int qb = (qt == 0) ? TQ - 1 : qt - 1;
        PopAcc<1> e;
        pop_epi_begin<1>(e);
        pop_chain<NM, 1>(a, b[qt], c0, accA, accB, P.dl, e);
        finish(std::integral_constant<int, qb>{}, e, (qt == 0) ? tB : t);
        pop_epi_begin<1>(e);
        if constexpr (qt + 2 == TQ)   // last chain of the tile
          pop_chain<NM, 1>(a, b[qt + 1], c0, accB, accA, P.dl, e, refill);
        else
          pop_chain<NM, 1>(a, b[qt + 1], c0, accB, accA, P.dl, e);
        finish(std::integral_constant<int, qt>{}, e, t);
      });
      keep_alive(c0);
      tB = t;
    };
    if constexpr (kSingleBuffer<NM>) {
      uint32_t e0 = entry(0);
      load_tile<NM>(A.img_r, A.norms_r, e0, lane, h, a0, n0);
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t e1 = entry(i + 1);
        compute(a0, n0, e0, e1);
        e0 = e1;
      }
    } else {
      s16x8 a1[NM];
      float4 n1[4];
      auto peek = [&](uint32_t i) { return list[i < cnt ? i : cnt - 1]; };
      uint32_t e0 = entry(0), e1;
      uint32_t l_next = peek(1);
      load_tile<NM>(A.img_r, A.norms_r, e0, lane, h, a0, n0);
      for (uint32_t i = 0; i < cnt; i += 2) {
        e1 = (uint32_t)__builtin_amdgcn_readfirstlane(l_next);
        l_next = peek(i + 2);
        load_tile<NM>(A.img_r, A.norms_r, e1, lane, h, a1, n1);
        compute(a0, n0, e0, e1);
        if (i + 1 < cnt) {
          e0 = (uint32_t)__builtin_amdgcn_readfirstlane(l_next);
          l_next = peek(i + 3);
          load_tile<NM>(A.img_r, A.norms_r, e0, lane, h, a0, n0);
          compute(a1, n1, e1, e0);
        }
      }
    }
    {  // drain: epilogue of the last pending chain of this round
      PopAcc<1> e;
      pop_epi_begin<1>(e);
      pop_epi<1, 0, 16>(accB, P.dl, e);
      finish(std::integral_constant<int, TQ - 1>{}, e, tB);
    }
  }
  if (lane == 0 && chains != 0u) {
    atomicAdd(A.chain_counter, (unsigned long long)chains);
    atomicAdd(A.chain_counter + kMfmaCtrPop, (unsigned long long)chains * NM);
  }
  flush_wave();

#pragma unroll
  for (int qt = 0; qt < TQ; ++qt) {
    const bool live = (livemask[qt] >> lane) & 1;
    const uint32_t total = cnt_q[qt] + (uint32_t)__shfl_xor((int)cnt_q[qt], 32, 64) + fix_tab[qt * 32 + c];
    if (h == 0 && live) {
      if (n_chunks == 1)
        pops[jq[qt]] = total;
      else if (total != 0u)
        atomicAdd(&pops[jq[qt]], total);   // pops was zero-filled by the caller
    }
  }
}

template <int S>
void pop_against_dispatch(const AgainstArgs& A, uint32_t n_cols, const Rad2& rad2, uint32_t* pops, hipStream_t s) {
  constexpr int TQ = tq_pop(S);
  const uint32_t waves = (A.T_q + TQ - 1) / TQ;
  if (waves == 0 || A.T_r == 0) return;
  const uint32_t wpb = waves_per_group(S, sweep_switches());
  const dim3 grid(grid_x8((waves + wpb - 1) / wpb),
                  pick_chunks(waves * TQ, TQ, kPopWaveTarget, A.T_r, pop_share_floor(A.T_r), (size_t)S * 1024 + 128)),
      block(64 * wpb);
  const size_t smem = wpb * (sizeof(uint32_t) * (kListCap + kWaveQueue + TQ * 32) + sizeof(float) * TQ * 32 * (size_t)n_cols);
  if (smem > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pop_against_kernel<S, TQ>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  timed_launch(0, s, [&] {
    hipLaunchKernelGGL((pop_against_kernel<S, TQ>), grid, block, smem, s, A, n_cols, rad2, pops);
  });
}

// (only the instances of the MFMA counts the library is built for -- DC_STEP_MASK, as in dc_mfma.hip -- exist)
template <int S>
void pop_against_step(const AgainstArgs& A, uint32_t n_cols, const Rad2& rad2, uint32_t* pops, hipStream_t s) {
  if constexpr (((DC_STEP_MASK >> (S - 1)) & 1u) != 0) pop_against_dispatch<S>(A, n_cols, rad2, pops, s);
}

}  // namespace

#define DC_FOR_EACH_S(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13)

void pop_against_sweep(const AgainstArgs& A, uint32_t n_cols, const Rad2& rad2, uint32_t* pops, hipStream_t s) {
  switch (nm_for((int)n_cols)) {
#define X_(SV)                                             \
  case SV:                                                 \
    pop_against_step<SV>(A, n_cols, rad2, pops, s);        \
    break;
    DC_FOR_EACH_S(X_)
#undef X_
    default:
      break;
  }
}

}  // namespace dc
