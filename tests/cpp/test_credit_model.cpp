// Host model of the reference-side credit network (clustering_amd/csrc/dc_credit.hpp): the SAME credit_slots and
// credit_network text the kernels compile, instantiated over a wave of 64 emulated lanes whose exchanges follow the ISA's
// description of the DPP controls and of v_permlane16_swap.  Checked against a plain column sum over the 32 lanes of each
// half-wave (tests/test_credit_model.py builds and runs this with g++; no GPU involved):
//   binary    every pattern of 16 elements with counts 0 or 6, (a) the same in all lanes -- all 32 x 16 counts at 6, sums of
//             192, among them -- and (b) in ONE lane of each half (every lane in turn, the two halves with different
//             patterns), the other lanes empty;
//   random    seeded inputs, counts 0 .. 6 drawn per (lane, element), the strings that carry a count chosen at random;
//   bounds    after every level no field exceeds the level's bound, the bound fits the field and nothing lies outside
//             the fields (so no field carries into its neighbour);
//   rows      the lanes that credit are 16 per half-wave and name, through credit_lane_row, each of the half's 16 rows of
//             the tile exactly once -- the row tile_row gives the element they hold.
#include "dc_credit.hpp"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Wave {
  std::array<uint32_t, 64> v;
  Wave() : v{} {}
  explicit Wave(uint32_t s) { v.fill(s); }
};
#define WAVE_OP(op)                                              \
  static inline Wave operator op(const Wave& a, const Wave& b) { \
    Wave r;                                                      \
    for (int i = 0; i < 64; ++i) r.v[i] = a.v[i] op b.v[i];      \
    return r;                                                    \
  }                                                              \
  static inline Wave operator op(const Wave& a, uint32_t s) {    \
    Wave r;                                                      \
    for (int i = 0; i < 64; ++i) r.v[i] = a.v[i] op s;           \
    return r;                                                    \
  }
WAVE_OP(+)
WAVE_OP(&)
WAVE_OP(|)
WAVE_OP(^)
WAVE_OP(>>)

static long long g_bound_failures = 0;
static uint32_t g_level_max[6] = {0, 0, 0, 0, 0, 0};

// source lane of a DPP control for destination lane i, -1: none (rows of 16 lanes, quads of 4)
static int dpp_source(int ctrl, int i) {
  const int row = i & ~15, l = i & 15;
  if (ctrl >= 0x000 && ctrl <= 0x0FF) return (i & ~3) + ((ctrl >> (2 * (i & 3))) & 3);   // quad_perm
  if (ctrl >= 0x101 && ctrl <= 0x10F) return (l + (ctrl & 15) < 16) ? row + l + (ctrl & 15) : -1;   // row_shl
  if (ctrl >= 0x111 && ctrl <= 0x11F) return (l - (ctrl & 15) >= 0) ? row + l - (ctrl & 15) : -1;   // row_shr
  if (ctrl >= 0x121 && ctrl <= 0x12F) return row + ((l - (ctrl & 15)) & 15);                        // row_ror
  if (ctrl == 0x140) return row + 15 - l;                                                           // row_mirror
  if (ctrl == 0x141) return row + (l & 8) + 7 - (l & 7);                                            // row_half_mirror
  std::fprintf(stderr, "DPP control %#x is not modelled\n", ctrl);
  std::exit(2);
}
// v_mov_b32_dpp: lanes outside the row / bank masks, and lanes without a source unless bound_ctrl, keep `old`
static Wave dpp(const Wave& old, const Wave& src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
  Wave r = old;
  for (int i = 0; i < 64; ++i) {
    if (!((row_mask >> (i >> 4)) & 1) || !((bank_mask >> ((i >> 2) & 3)) & 1)) continue;
    const int s = dpp_source(ctrl, i);
    if (s >= 0)
      r.v[i] = src.v[s];
    else if (bound_ctrl)
      r.v[i] = 0;
  }
  return r;
}

struct CreditModel {
  Wave xor3(const Wave& a, const Wave& b, const Wave& c) const { return a ^ b ^ c; }
  Wave maj3(const Wave& a, const Wave& b, const Wave& c) const { return (a & b) | (a & c) | (b & c); }
  Wave pick_bits(uint32_t m, const Wave& a, const Wave& b) const { return (a & m) | (b & ~m); }
  // v_permlane16_swap vdst, src: the odd rows of vdst change places with the even rows of src
  void swap16(Wave& a, Wave& b) const {
    for (int i = 0; i < 64; ++i)
      if ((i >> 4) & 1) {
        const uint32_t t = a.v[i];
        a.v[i] = b.v[i - 16];
        b.v[i - 16] = t;
      }
  }
  template <int CTRL>
  Wave take(const Wave& v) const {
    return dpp(Wave(0u), v, CTRL, 0xF, 0xF, true);
  }
  template <int BANKS>
  Wave pick(const Wave& u, const Wave& v) const {
    return dpp(u, v, 0xE4, 0xF, BANKS, false);
  }
  void level(int n, const Wave& v, int width, uint32_t bound) const {
    if (bound >= (1u << width)) ++g_bound_failures;
    for (int i = 0; i < 64; ++i)
      for (int b = 0; b < 32; b += width) {
        const uint32_t f = (v.v[i] >> b) & ((1u << width) - 1u);
        if (f > bound) ++g_bound_failures;
        if (f > g_level_max[n]) g_level_max[n] = f;
      }
  }
};

static long long g_cases = 0, g_mismatches = 0;

// counts[lane][r] in 0 .. 6; which[lane][r]: bit q set -> string q carries the element (popcount = the count)
static void run_case(const uint8_t (&which)[64][16]) {
  Wave sb[6];
  unsigned want[2][16] = {};
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 16; ++r) {
      for (int q = 0; q < 6; ++q)
        if ((which[lane][r] >> q) & 1) {
          sb[q].v[lane] |= 1u << (31 - 2 * r);
          ++want[lane >> 5][r];
        }
    }
  // (the bits beside the signs are whatever the classification left there: the network must not read them)
  for (int q = 0; q < 6; ++q)
    for (int lane = 0; lane < 64; ++lane) sb[q].v[lane] |= (0x9E3779B9u * (uint32_t)(g_cases + 64 * q + lane + 1)) & 0x55555555u;
  Wave A, B;
  const CreditModel X;
  credit_slots<6>(sb, A, B, X);
  const Wave w = credit_network(A, B, X);
  for (int lane = 0; lane < 64; ++lane) {
    if (!credit_lane_active(lane)) continue;
    const uint32_t cnt = (w.v[lane] >> credit_lane_shift(lane)) & 0xFFu;
    if (cnt != want[lane >> 5][credit_lane_element(lane)]) ++g_mismatches;
  }
  ++g_cases;
}

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

int main(int argc, char** argv) {
  const long n_random = argc > 1 ? std::atol(argv[1]) : 300000;

  // rows: 16 crediting lanes per half, each row of the half once, and it is the row of the element the lane holds
  int seen[2][32] = {};
  int active[2] = {0, 0};
  long long row_failures = 0;
  for (int lane = 0; lane < 64; ++lane) {
    if (!credit_lane_active(lane)) continue;
    const int h = lane >> 5, r = credit_lane_element(lane);
    ++active[h];
    if (r < 0 || r > 15) ++row_failures;
    const uint32_t row = credit_lane_row(lane);
    if (row != (uint32_t)((r & 3) + 8 * (r >> 2) + 4 * h) || row >= 32u) ++row_failures;
    if (credit_lane_shift(lane) > 24u || credit_lane_shift(lane) % 8u) ++row_failures;
    ++seen[h][row & 31];
  }
  for (int h = 0; h < 2; ++h) {
    if (active[h] != 16) ++row_failures;
    for (int row = 0; row < 32; ++row)
      if (seen[h][row] != (((row >> 2) & 1) == h ? 1 : 0)) ++row_failures;   // half h owns the rows with bit 2 = h
  }
  int both[32] = {};
  for (int h = 0; h < 2; ++h)
    for (int row = 0; row < 32; ++row) both[row] += seen[h][row];
  for (int row = 0; row < 32; ++row)
    if (both[row] != 1) ++row_failures;

  static uint8_t which[64][16];
  // binary (a): the same pattern in every lane
  for (uint32_t pat = 0; pat < 65536u; ++pat) {
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 16; ++r) which[lane][r] = ((pat >> r) & 1) ? 0x3F : 0;
    run_case(which);
  }
  // binary (b): one lane of each half carries a pattern (the upper half another one), every lane in turn
  for (uint32_t pat = 0; pat < 65536u; ++pat) {
    const int c = (int)(pat & 31u);   // every (pattern, lane) pair would be 32 x as many: the lane cycles with the pattern,
    for (int pass = 0; pass < 2; ++pass) {   // and a second pass pairs each pattern with the lane 16 + ... away as well
      const int cc = (c + 16 * pass + (int)((pat >> 5) & 15u)) & 31;
      std::memset(which, 0, sizeof(which));
      const uint32_t pat_hi = (pat * 40503u + 1u) & 0xFFFFu;
      for (int r = 0; r < 16; ++r) {
        which[cc][r] = ((pat >> r) & 1) ? 0x3F : 0;
        which[32 + (31 - cc)][r] = ((pat_hi >> r) & 1) ? 0x3F : 0;
      }
      run_case(which);
    }
  }
  // ... and every lane with every single element (a one-hot lane reaches each row through its own path)
  for (int c = 0; c < 32; ++c)
    for (int r = 0; r < 16; ++r) {
      std::memset(which, 0, sizeof(which));
      which[c][r] = 0x3F;
      which[32 + c][15 - r] = 0x3F;
      run_case(which);
    }
  const long long n_binary = g_cases;
  // random: counts 0 .. 6, carried by a random choice of the six strings
  for (long k = 0; k < n_random; ++k) {
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 16; ++r) {
        const uint32_t x = rnd();
        const int cnt = (int)(x % 7u);
        uint8_t m = 0;
        for (int left = cnt, q = 0; q < 6; ++q)   // cnt of the six strings, chosen uniformly
          if ((rnd() % (uint32_t)(6 - q)) < (uint32_t)left) {
            m |= (uint8_t)(1u << q);
            --left;
          }
        which[lane][r] = m;
      }
    run_case(which);
  }
  std::printf("binary %lld random %lld mismatches %lld bound_failures %lld row_failures %lld level_max %u %u %u %u %u %u\n",
              n_binary, g_cases - n_binary, g_mismatches, g_bound_failures, row_failures, g_level_max[0], g_level_max[1],
              g_level_max[2], g_level_max[3], g_level_max[4], g_level_max[5]);
  const bool ok = g_mismatches == 0 && g_bound_failures == 0 && row_failures == 0;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
