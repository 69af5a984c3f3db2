// The lane network behind the reference-side credit of the symmetric population sweeps: per reference
// row of a 32 x 32 tile, the sum over the 32 query lanes of a half-wave of the number of "inside" chains (0 .. TQ <= 6
// per lane and element).  Plain C++ over a value type V and an exchange functor X, so that the same text compiles
//   for the device: V = uint32_t, X = the DPP / permlane form (dc_mfma_kernels.hpp: CreditDpp), and
//   for the host:   V = 64 emulated lanes, X = the same exchanges on arrays (tests/cpp/test_credit_model.cpp),
// which is what lets the network be checked exhaustively without a GPU.
//
// Layout.  Lane = 32 h + c holds, of the accumulator of query c, the 16 elements r = 4 g + j <-> row 8 g + 4 h + j of
// the tile (tile_row).  The in-lane stage (credit_slots) leaves the counts in two words of eight 4-bit slots:
//   A slot s = element 15 - 2 s,   B slot s = element 14 - 2 s.
// The network is a halving butterfly for as long as halving pays, i.e. while a lane carries more than one word or a
// level has to widen its fields; after that all fields of a lane fit ONE word whose bytes cannot overflow (<= 192), a
// level is one add whichever way it is taken, and keeping all four bytes spares the select:
//   level  partner  exchange                      lane keeps                               fields       bound
//   1      c ^ 16   permlane16 swap of (A, B)     b4 = 0: A, b4 = 1: B                     8 x 4 bit    12
//   2      c ^ 8    row_ror:8, bank-masked pick   b3 = 0: even slots, b3 = 1: odd slots    4 x 8 bit    24
//   3      c ^ 1    quad_perm:[1,0,3,2]           all four bytes                           4 x 8 bit    48
//   4      c ^ 2    quad_perm:[2,3,0,1]           all four bytes                           4 x 8 bit    96
//   5      c ^ 7    row_half_mirror               all four bytes                           4 x 8 bit    192
// (b3, b4: bits 3 and 4 of c.  After levels 3 and 4 the lanes of a quad agree, so c ^ 7 is as good as c ^ 4.)
// After level 2 byte k of a lane is slot 2 k + b3 of word b4, i.e. element 15 - 4 k - 2 b3 - b4; levels 3 - 5 sum over
// the eight lanes that share (b3, b4).  Of those eight, the four with bit 2 of c clear credit one byte each, k = c & 3:
//   lane c (bit 2 clear) credits element r = 15 - 4 (c & 3) - 2 b3 - b4, i.e. row 8 (3 - (c & 3)) + 4 h + 3 - 2 b3 - b4
// -- 16 lanes per half-wave, each of a half's 16 rows exactly once, with nothing staged outside the registers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_CREDIT_FN __host__ __device__ __forceinline__
#else
#define DC_CREDIT_FN inline
#endif

// row (within its tile) held by accumulator register r of a lane in half h
DC_CREDIT_FN constexpr uint32_t tile_row_local(int r, int h) { return (uint32_t)((r & 3) + 8 * (r >> 2) + 4 * h); }

// DPP controls of the exchanges (the host emulation decodes the same numbers)
constexpr int kDppQuadXor1 = 0xB1;        // quad_perm:[1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;        // quad_perm:[2,3,0,1]
constexpr int kDppRowRor8 = 0x128;        // row_ror:8
constexpr int kDppRowHalfMirror = 0x141;  // row_half_mirror
constexpr int kCreditOddSlotBanks = 0xC;  // DPP banks (groups of four lanes of a row) with bit 3 of the lane set

// the lanes that credit, the byte they take and the element / row it belongs to (lane = 32 h + c)
DC_CREDIT_FN constexpr bool credit_lane_active(int lane) { return (lane & 4) == 0; }
DC_CREDIT_FN constexpr uint32_t credit_lane_shift(int lane) { return 8u * (uint32_t)(lane & 3); }
DC_CREDIT_FN constexpr int credit_lane_element(int lane) {
  return 15 - 4 * (lane & 3) - 2 * ((lane >> 3) & 1) - ((lane >> 4) & 1);
}
DC_CREDIT_FN constexpr uint32_t credit_lane_row(int lane) { return tile_row_local(credit_lane_element(lane), (lane >> 5) & 1); }

// in-lane stage: the sign bits (bit 31 - 2 r: element r is inside) of TQ strings add up bit-sliced, three strings at a
// time (X::xor3 / X::maj3: one three-input bit operation each on the device) into 2-bit fields; the fields of the groups
// of three are added in 4-bit slots
template <int TQ, class V, class X>
DC_CREDIT_FN void credit_slots(const V (&sb)[TQ], V& A, V& B, const X& x3) {
  static_assert(TQ >= 1 && TQ <= 6, "4-bit slots hold the sums of two groups of three strings over two lanes");
  A = V(0u);
  B = V(0u);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int g = 0; g < TQ; g += 3) {
    const V a = sb[g], b = (g + 1 < TQ) ? sb[g + 1] : V(0u), c = (g + 2 < TQ) ? sb[g + 2] : V(0u);
    const V lo = x3.xor3(a, b, c), hi = x3.maj3(a, b, c);             // valid at the sign positions (odd bits)
    const V x = x3.pick_bits(0xAAAAAAAAu, hi, lo >> 1);               // element r: 0..3 at bits 31-2r, 30-2r
    A = A + (x & 0x33333333u);
    B = B + ((x >> 2) & 0x33333333u);
  }
}

// the lane network: A, B as credit_slots leaves them (slots <= 6); returns the word whose byte credit_lane_shift(lane) / 8
// is, in the lanes with credit_lane_active, the sum of element credit_lane_element(lane) over the 32 lanes of the half.
//   X::xor3, X::maj3(a,b,c)  a ^ b ^ c and (a & b) | (a & c) | (b & c)   (credit_slots)
//   X::pick_bits(m, a, b)    (a & m) | (b & ~m), m a constant                    (credit_slots)
//   X::swap16(a, b)          rows 1 and 3 of a change places with rows 0 and 2 of b (rows of 16 lanes)
//   X::take<CTRL>(v)         v of the lane the DPP control names
//   X::pick<BANKS>(u, v)     v in the lanes of the banks BANKS, u elsewhere
//   X::level(n, v, w, b)     a hook for the model: level n has left fields of w bits in v, none above b (no-op on the device)
template <class V, class X>
DC_CREDIT_FN V credit_network(V A, V B, const X& x) {
  x.level(0, A, 4, 6u);
  x.level(0, B, 4, 6u);
  x.swap16(A, B);
  const V n = A + B;
  x.level(1, n, 4, 12u);
  V even = n & 0x0F0F0F0Fu, odd = (n >> 4) & 0x0F0F0F0Fu;
  even = even + x.template take<kDppRowRor8>(even);
  odd = odd + x.template take<kDppRowRor8>(odd);
  V w = x.template pick<kCreditOddSlotBanks>(even, odd);
  x.level(2, w, 8, 24u);
  w = w + x.template take<kDppQuadXor1>(w);
  x.level(3, w, 8, 48u);
  w = w + x.template take<kDppQuadXor2>(w);
  x.level(4, w, 8, 96u);
  w = w + x.template take<kDppRowHalfMirror>(w);
  x.level(5, w, 8, 192u);
  return w;
}
