// Host-side check of the resident reference's workspace arithmetic over BOTH wide kinds (dc_mfma_wide.hip
// wide_reference_layout, wide_reference_workspace_bytes, xwide_reference_workspace_bytes): rows of
// 65..256 columns, whose byte offsets are pinned to what they were before the third kind existed, and rows of 257..1024,
// whose resident region starts behind the [1024] sums and means of that layout.  No device is touched: nothing here
// launches or allocates (tests/test_reference_xwide_layout.py runs it; it also builds under the host sanitizers,
// -Xarch_host -fsanitize=address,undefined).
#include <cstdio>
#include <vector>

#include "dc_mfma_wide.hip"

namespace dc {
void sweep_timer_mark(int, bool, hipStream_t) {}   // (dc_mfma.hip's, which this program does not link: nothing is launched here)
}  // namespace dc
using namespace dc;

static int fails = 0;
#define CHECK(c)                                                                                              \
  do {                                                                                                        \
    if (!(c)) {                                                                                               \
      ++fails;                                                                                                \
      std::printf("FAILED %s (line %d) n_r=%zu D=%zu max_batch=%zu n_q=%zu\n", #c, __LINE__, n_r, D, n_b, n_q); \
    }                                                                                                         \
  } while (0)

struct Region {
  size_t off, bytes;
};

// offsets of the 65..256 layouts as they were before this kind was added (bytes): every one must stay what it is
struct Pinned {
  size_t n_r, D, n_b;
  size_t img_a, norms, perm_r, coords_r, img_b, coords_q, cnt, keys, sort, total;
};
static const Pinned kPinned[] = {
    {1, 65, 1, 4096, 57344, 57856, 58112, 59648, 113408, 114176, 114944, 115712, 118272},
    {1500, 100, 300, 4096, 937984, 944128, 950272, 1563136, 1802752, 1923072, 1934336, 1952768, 1967104},
    {1500, 256, 129, 4096, 2412544, 2418688, 2424832, 3973632, 4378112, 4510464, 4515840, 4534272, 4548608},
    {8320, 255, 1100, 4096, 12783616, 12816896, 12850176, 21404928, 23196672, 24318976, 24359168, 24459008, 24531712},
    {129, 256, 4000, 4096, 405504, 406528, 407296, 541440, 7044096, 11140608, 11285248, 11333632, 11368960},
};

int main() {
  const std::vector<size_t> refs = {1, 127, 128, 129, 1500, 8320};
  const std::vector<size_t> batches = {1, 127, 128, 129, 1100, 5000};
  const std::vector<size_t> cols = {65, 256, 257, 258, 400, 401, 512, 1023, 1024};
  size_t checked = 0;
  for (size_t D : cols)
    for (size_t n_r : refs)
      for (size_t n_b : batches) {
        size_t n_q = n_b;
        const bool xw = D > kWideMaxCols;
        const WideReferenceLayout R = wide_reference_layout(n_r, D, n_b);
        const WideCrossPrunedLayout& P = R.P;
        const WideLayout& L = P.L;
        const size_t n_max = n_b > n_r ? n_b : n_r, tile_bytes = (size_t)16 * 64 * L.NM;
        CHECK(L.NM == (uint32_t)nm_for((int)D) && L.Tp % kWideBlockTiles == 0 && L.Tqp % kWideBlockTiles == 0);
        CHECK(P.blocks_r == (n_r + 127) / 128 && P.blocks_q == (n_b + 127) / 128);
        // the head: sums [cols of the family] doubles behind the header, means [cols of the family] floats behind them, and
        // the resident region never before the end of the means
        const size_t head = xw ? kXWideMaxCols : kWideMaxCols;
        CHECK(D <= head && wide_off_means(D) == kWideOffSums + 8 * head && wide_off_means(D) >= kWideOffSums + 8 * D);
        CHECK(wide_off_images(D) == wide_off_means(D) + 4 * head && wide_off_images(D) >= wide_off_means(D) + 4 * D);
        CHECK(wide_off_images(D) == (xw ? (size_t)13312 : (size_t)4096) && (xw || wide_off_images(D) == kWideOffImages));
        CHECK(R.resident_begin == wide_off_images(D) && L.off_img_a == R.resident_begin);
        const Region resident[] = {{L.off_img_a, tile_bytes * L.Tp},    {L.off_norms, 4 * 32 * (size_t)L.Tp},
                                   {P.off_perm_r, 4 * n_r},             {P.off_coords_r, 4 * n_r * D},
                                   {P.off_boxes_r, 16 * (size_t)P.blocks_r}, {R.N.off_fe_r, 4 * n_r},
                                   {R.N.off_fe_min_r, 4 * (size_t)P.blocks_r}, {R.off_fe_row, 4 * n_r}};
        const Region batch[] = {{L.off_img_b, tile_bytes * L.Tqp},       {L.off_merge, 16 * n_b},
                                {P.off_perm_q, 4 * n_b},                 {P.off_coords_q, 4 * n_b * D},
                                {P.off_boxes_q, 16 * (size_t)P.blocks_q}, {P.off_cnt, 4 * (size_t)kMaxRadiiPerLaunch * n_b},
                                {R.N.off_fe_q, 4 * n_b},                 {R.N.off_qwords, 16 * (size_t)P.blocks_q}};
        const Region scratch[] = {{P.off_keys, 4 * n_max}, {P.off_keys_o, 4 * n_max}, {P.off_vals, 4 * n_max}, {P.off_sort, sort_temp_bytes(n_max)}};
        // every array inside the total, in the order it is laid out, none over another; the head in front of all
        size_t end = wide_off_images(D);
        for (const Region& r : resident) {
          CHECK(r.off % 256 == 0 && r.off >= end && r.off + r.bytes <= R.resident_end);
          end = r.off + r.bytes;
        }
        // the resident, the batch and the scratch region are disjoint, in that order
        CHECK(R.resident_end <= R.batch_begin && R.batch_begin <= R.batch_end && R.batch_end <= P.total);
        end = R.batch_begin;
        for (const Region& r : batch) {
          CHECK(r.off % 256 == 0 && r.off >= end && r.off + r.bytes <= R.batch_end);
          end = r.off + r.bytes;
        }
        end = R.batch_end;
        for (const Region& r : scratch) {
          CHECK(r.off % 256 == 0 && r.off >= end && r.off + r.bytes <= P.total);
          end = r.off + r.bytes;
        }
        CHECK(P.total % 256 == 0 && L.total == P.total);
        // each kind's size function answers for its widths alone
        CHECK(wide_reference_workspace_bytes(n_r, D, n_b) == (xw ? 0 : P.total));
        CHECK(xwide_reference_workspace_bytes(n_r, D, n_b) == (xw ? P.total : 0));
        CHECK(P.sort_bytes >= sort_temp_bytes(n_b) && P.sort_bytes >= sort_temp_bytes(n_r));
        CHECK(4 * (kWideHdrResMref + 1) <= kHdrBytes && kWideHdrResFlagRef > kWideHdrOrderHash + 1 && R.N.off_flag_q == 4 * kWideHdrResFlagFeQuery);
        // every batch the handle takes: its images, words per block and counts fit where the launcher puts them, and the
        // unit map is the pruned cross sweep's of the same shape
        for (size_t q : {(size_t)1, n_b / 2 + 1, n_b}) {
          n_q = q;
          const uint32_t blocks_q = (uint32_t)((n_q + kWideBlockRows - 1) / kWideBlockRows);
          CHECK(wide_pad_tiles((uint32_t)((n_q + 31) / 32)) <= L.Tqp && blocks_q <= P.blocks_q);
          // the words per query block as nn_wide_cross_pruned forms their pointers: fe_max_q at off_qwords, far2 (nn, hd)
          // P.blocks_q words behind it and 2 P.blocks_q long, the seed behind that; a batch writes blocks_q words of each
          const size_t w_fe_max = R.N.off_qwords, w_far2 = w_fe_max + 4 * (size_t)P.blocks_q, w_seed = w_far2 + 4 * 2 * (size_t)P.blocks_q;
          CHECK(w_fe_max + 4 * (size_t)blocks_q <= w_far2 && w_far2 + 4 * ((size_t)P.blocks_q + blocks_q) <= w_seed);
          CHECK(w_seed + 4 * (size_t)blocks_q <= R.N.off_qwords + 16 * (size_t)P.blocks_q && w_seed + 4 * (size_t)blocks_q <= R.batch_end);
          CHECK(R.N.off_fe_min_r + 4 * (size_t)P.blocks_r <= R.off_fe_row && R.N.off_fe_r + 4 * n_r <= R.N.off_fe_min_r);
          const WideCrossPrunedLayout C = wide_cross_pruned_layout(n_q, n_r, D);
          CHECK(C.L.Tp == L.Tp && C.L.NM == L.NM && C.blocks_r == P.blocks_r && C.L.off_img_a == L.off_img_a);
          const uint32_t shares = wide_shares(P.blocks_r), grid = wide_grid_size(blocks_q, shares);
          CHECK(shares == wide_shares(C.blocks_r) && grid == wide_grid_size((uint32_t)((n_q + 127) / 128), shares) && grid % 512 == 0);
          if (blocks_q <= 16) {
            std::vector<char> seen((size_t)blocks_q * shares, 0);
            for (uint32_t id = 0; id < grid; ++id) {
              const WideUnit u = wide_unit(id, shares);
              CHECK(u.share < shares);
              if (u.q_block < blocks_q) {
                CHECK(!seen[(size_t)u.q_block * shares + u.share]);
                seen[(size_t)u.q_block * shares + u.share] = 1;
              }
            }
            for (char c : seen) CHECK(c == 1);
          }
          ++checked;
        }
      }
  // up to 256 columns: the recorded offsets
  for (const Pinned& k : kPinned) {
    const size_t n_r = k.n_r, D = k.D, n_b = k.n_b, n_q = 0;
    const WideReferenceLayout R = wide_reference_layout(n_r, D, n_b);
    CHECK(R.P.L.off_img_a == k.img_a && R.P.L.off_norms == k.norms && R.P.off_perm_r == k.perm_r && R.P.off_coords_r == k.coords_r);
    CHECK(R.P.L.off_img_b == k.img_b && R.P.off_coords_q == k.coords_q && R.P.off_cnt == k.cnt && R.P.off_keys == k.keys);
    CHECK(R.P.off_sort == k.sort && R.P.total == k.total && wide_reference_workspace_bytes(n_r, D, n_b) == k.total);
    ++checked;
  }
  // monotone in each argument; zero outside the kind's widths and for a zero count
  for (size_t D : {(size_t)257, (size_t)512, (size_t)1024}) {
    size_t n_r = 0, n_b = 0, n_q = 0;
    for (size_t fixed : {(size_t)1, (size_t)300, (size_t)20000}) {
      size_t last_r = 0, last_b = 0;
      for (size_t n : refs) {
        n_r = n, n_b = fixed;
        const size_t a = xwide_reference_workspace_bytes(n, D, fixed), b = xwide_reference_workspace_bytes(fixed, D, n);
        CHECK(a >= last_r && b >= last_b && a > 0 && b > 0);
        last_r = a, last_b = b;
      }
    }
    CHECK(xwide_reference_workspace_bytes(0, D, 100) == 0 && xwide_reference_workspace_bytes(100, D, 0) == 0);
    CHECK(xwide_reference_workspace_bytes(100, D, 100) >= xwide_reference_workspace_bytes(100, D - 1 < 257 ? 257 : D - 1, 100));
  }
  for (size_t D : {(size_t)0, (size_t)1, (size_t)64, (size_t)65, (size_t)256, (size_t)1025}) {
    size_t n_r = 1000, n_b = 1000, n_q = 0;
    CHECK(xwide_reference_workspace_bytes(n_r, D, n_b) == 0);
  }
  std::printf("%s %zu layouts\n", fails ? "FAILED" : "ok", checked);
  return fails ? 1 : 0;
}
