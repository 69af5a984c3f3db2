// dc_reference.hpp -- the resident reference of the pruned cross sweeps for rows of 1..64 columns (dc_hip_reference_*,
// DESIGN.md 4.29): the kernels of its preparation (included by dc_mfma.hip inside namespace dc::{anonymous}, behind
// dc_prep.hpp, whose orders it builds).  The sweeps are pop_against_kernel and nn_against_kernel as they stand.
//
// The statistics cannot depend on a batch:
//   origin   the column means of the reference (colsum_kernel, mean_kernel over R alone)
//   extent   M_res = 4 M_ref, M_ref = the largest |x - mean|^2 of the reference as rowstats_kernel forms it.  M_res
//            stands in header word 0 and kHdrMused, where M stands: guard_band, pop_setup and the image builder form
//            everything from it.  The band (dc_mfma_kernels.hpp, "guard band") asks of the data only that M bounds
//            |x'|^2 = |x - origin|^2 of every row of BOTH operands, measured from the one origin: the reference meets
//            that with room (M_ref <= M_res), and a batch by the test of ref_gate_kernel -- a batch with a row beyond
//            M_res is flagged and answered by the direct kernels.  A query up to twice as far from the origin as the
//            farthest reference frame runs on the matrix cores.
//   grid     header words 8..11 hold the reference's extent in columns 0 / 1 alone.  A row outside it is clamped into an
//            edge cell (against_key_kernel's arithmetic); its tile's box is formed from its own floats
//            (against_rows_kernel), so the order may be worse for such a query and the pruning stays exact.
//   scales   two: pick_scale_pop(M_res, fl32(max_radius^2), D) for the population sweep -- the largest radius any
//            population call of the handle may use is fixed when it is opened, because the resident A image is built at
//            that scale -- and pick_scale_nn(M_res) for the neighbour sweep.  Both are kept in the resident words; the
//            arm kernel copies the one a sweep runs under into words 20..24.
#pragma once

// The resident words: kRefWordsBytes behind the header, addressed from the header's pointer.  The four flags are kept
// apart; header word 1 -- the word every gate reads -- is formed from them in front of every sweep (ref_arm_kernel).
constexpr uint32_t kRefWords = (uint32_t)(kHdrBytes / 4);
constexpr uint32_t kRefFlagRef = kRefWords + 0;      // the reference holds a non-finite / overflow-prone row, or 4 M_ref is beyond kNormLimit
constexpr uint32_t kRefFlagBatch = kRefWords + 1;    // the staged batch holds a row that is non-finite or beyond M_res
constexpr uint32_t kRefAnswered = kRefWords + 2;     // who answered the last sweep: 0 the matrix cores, 1..3 the direct kernels (dc_density.h)
constexpr uint32_t kRefMref = kRefWords + 3;         // M_ref (float bits)
constexpr uint32_t kRefScalePop = kRefWords + 8;     // [5] the population scale, as words 20..24 hold a scale
constexpr uint32_t kRefScaleNn = kRefWords + 16;     // [5] the neighbour scale
// fe_key_kernel's view of a header (word 1: bit 2 for a NaN, words 12 / 13: the range), for the free energies of the
// reference and for those of the last neighbour sweep's queries
constexpr uint32_t kRefFeRefHdr = kRefWords + 32, kRefFeQueryHdr = kRefWords + 64;
constexpr uint32_t kRefFlagFeRef = kRefFeRefHdr + 1, kRefFlagFeQuery = kRefFeQueryHdr + 1;
static_assert(4 * (size_t)(kRefFeQueryHdr + 14) <= kHdrBytes + kRefWordsBytes && kRefScaleNn + 5 <= kRefFeRefHdr,
              "the resident words lie inside their region, none over another");

// behind the reference's statistics (word 0 = M_ref, word 1 = its flag): M_res in words 0 and kHdrMused, the flag in a
// word of its own, both scales
__global__ void ref_scale_kernel(uint32_t* __restrict__ hdr, float r2max, uint32_t D) {
  const float M_ref = __uint_as_float(hdr[0]), M_res = 4.0f * M_ref;
  const bool flagged = hdr[1] != 0u || !(M_res <= kNormLimit);
  const float M = (M_res <= kNormLimit) ? M_res : M_ref;   // (a flagged reference is never swept: any finite extent serves)
  hdr[kRefMref] = __float_as_uint(M_ref);
  hdr[kRefFlagRef] = flagged ? 1u : 0u;
  hdr[0] = __float_as_uint(M);
  hdr[kHdrMused] = __float_as_uint(M);
  hdr[1] = flagged ? 1u : 0u;
  const ScaleExp e[2] = {pick_scale_pop(M, r2max, (int)D), pick_scale_nn(M)};
  const uint32_t at[2] = {kRefScalePop, kRefScaleNn};
  for (int k = 0; k < 2; ++k) {
    hdr[at[k] + 0] = __float_as_uint(e[k].c);
    hdr[at[k] + 1] = __float_as_uint(e[k].s2);
    hdr[at[k] + 2] = (uint32_t)e[k].g;
    hdr[at[k] + 3] = (uint32_t)e[k].a;
    hdr[at[k] + 4] = (uint32_t)e[k].rounded;
  }
}

// In front of every sweep, and of every image built at a sweep's scale (which: 0 the population sweep, 1 the
// neighbour sweep; with_fe: a neighbour sweep that reads free energies).  Word 1 from the four flags, who answers, the
// sweep's scale in words 20..24, the range of the reference's free energies in words 12 / 13, the counters of both
// sweeps and the share word from zero: nothing is left over from the sweep before.
__global__ void ref_arm_kernel(uint32_t* __restrict__ hdr, uint32_t which, uint32_t with_fe) {
  const uint32_t t = threadIdx.x;
  if (t >= 2u && t <= 7u) hdr[t] = 0u;   // words 2..7: evaluated tile pairs of either sweep, the population sweep's MFMAs
  if (t < 2u) hdr[kHdrMfmaNn + t] = 0u;
  if (t < 5u) hdr[kHdrScale + t] = hdr[(which ? kRefScaleNn : kRefScalePop) + t];
  if (t == 0u) {
    const bool ref = hdr[kRefFlagRef] != 0u, batch = hdr[kRefFlagBatch] != 0u;
    const bool fe = with_fe != 0u && (hdr[kRefFlagFeRef] | hdr[kRefFlagFeQuery]) != 0u;
    hdr[1] = (ref || batch || fe) ? 1u : 0u;
    hdr[kRefAnswered] = ref ? 1u : (batch ? 2u : (fe ? 3u : 0u));
    hdr[kHdrShares] = 0u;
    hdr[kHdrShift] = 0u;
    hdr[kHdrOpen] = 0u;
    hdr[12] = with_fe ? hdr[kRefFeRefHdr + 12] : 0u;
    hdr[13] = with_fe ? hdr[kRefFeRefHdr + 13] : 0u;
  }
}

// in front of a pass of fe_key_kernel over view `at` of the resident words (its words are raised with atomics)
__global__ void ref_fe_reset_kernel(uint32_t* __restrict__ hdr, uint32_t at) {
  hdr[at + 1] = 0u;
  hdr[at + 12] = 0u;
  hdr[at + 13] = 0u;
}

// The gate of a batch, its ONE pass over the rows: a row per lane, read where it lies, as rowstats_kernel reads the
// reference -- consecutive lanes read consecutive rows, so the D loads of a wave walk the same 64 D floats and meet in
// the vector cache; several lanes per row would have to reduce across lanes and sum in another order.  |x - mean|^2 in
// double, summed exactly as rowstats_kernel sums it (the pair loads for an even D and 8-byte aligned rows included), so
// the float it rounds to is the one M_ref was taken from.  The batch's flag is raised by a row that is non-finite,
// beyond kNormLimit or beyond M_res (header word 0).  From columns 0 / 1 of the row: its cell key on the reference's
// population grid and on its neighbour grid (against_key_kernel's arithmetic, clamped into the edge cells), each with
// the row's number as the value of its sort; and the presets of both query orders (kInvalidFrame on all n_pos
// positions: the sorts write the real entries over the first of them).
// Stands in for two colsum, one mean, two rowstats and two against_key launches of a per-call preparation.
__global__ __launch_bounds__(256) void ref_gate_kernel(const float* __restrict__ coords, uint32_t n_rows, uint32_t D,
                                                       const float* __restrict__ means, uint32_t* __restrict__ hdr,
                                                       uint32_t n_ref, float pop_cell_frames, float nn_cell_frames,
                                                       uint32_t* __restrict__ keys_pop, uint32_t* __restrict__ vals_pop,
                                                       uint32_t* __restrict__ keys_nn, uint32_t* __restrict__ vals_nn,
                                                       uint32_t* __restrict__ perm_pop, uint32_t* __restrict__ perm_nn,
                                                       uint32_t n_pos) {
  __shared__ float mu[kMaxCols];
  if (threadIdx.x < D) mu[threadIdx.x] = means[threadIdx.x];
  __syncthreads();
  const float M_res = __uint_as_float(hdr[0]);
  const AgainstGrid g_pop = against_grid(hdr, n_ref, pop_cell_frames), g_nn = against_grid(hdr, n_ref, nn_cell_frames);
  auto key_of = [](const AgainstGrid& g, float x, float y) -> uint32_t {
    if (!(fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX)) return 0u;   // (a non-finite row: the batch is flagged)
    const uint32_t bx = (uint32_t)fminf(fmaxf((x - g.lo0) / g.cell, 0.0f), 4000.0f);
    const uint32_t by = min((uint32_t)fminf(fmaxf((y - g.lo1) / g.cell, 0.0f), 4000.0f), g.ny - 1u);
    return bx * g.ny + ((bx & 1u) ? g.ny - 1u - by : by);
  };
  const bool pairs = (D % 2u == 0) && ((reinterpret_cast<uintptr_t>(coords) & 7u) == 0);
  bool bad = false;
  for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < n_pos; row += gridDim.x * blockDim.x) {
    perm_pop[row] = kInvalidFrame;
    perm_nn[row] = kInvalidFrame;
    if (row >= n_rows) continue;
    const float* x = coords + (size_t)row * D;
    double nrm = 0.0;
    float c0 = 0.0f, c1 = 0.0f;
    if (pairs) {
      const float2* x2 = reinterpret_cast<const float2*>(x);
      for (uint32_t k = 0; k < D; k += 2) {
        const float2 v = x2[k >> 1];
        if (k == 0) {
          c0 = v.x;
          c1 = v.y;
        }
        const float a = v.x - mu[k], b = v.y - mu[k + 1];
        nrm += (double)a * (double)a;
        nrm += (double)b * (double)b;
      }
    } else {
      c0 = x[0];
      if (D > 1) c1 = x[1];
      for (uint32_t k = 0; k < D; ++k) {
        const float v = x[k] - mu[k];
        nrm += (double)v * (double)v;
      }
    }
    const float nf = (float)nrm;
    bad = bad | !(nf <= kNormLimit) | !(nf <= M_res);
    keys_pop[row] = key_of(g_pop, c0, c1);
    vals_pop[row] = row;
    keys_nn[row] = key_of(g_nn, c0, c1);
    vals_nn[row] = row;
  }
  if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(hdr + kRefFlagBatch, 1u);
}
