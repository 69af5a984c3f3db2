// Host-side check of the resident reference's workspace arithmetic (dc_mfma_wide.hip wide_reference_layout,
// wide_reference_workspace_bytes) under the host sanitizers.  No device is touched: nothing here launches or allocates.
//   cd clustering_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I. -I../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -o /tmp/reference_wide_layout_check ../../scratch/reference_wide_layout_check.hip dc_sort.hip && /tmp/reference_wide_layout_check
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

int main() {
  const std::vector<size_t> refs = {1, 2, 127, 128, 129, 1000, 1500, 8320, 20000, 200000, 4000000};
  const std::vector<size_t> batches = {1, 31, 32, 33, 127, 128, 129, 300, 1100, 20000, 300000};
  const std::vector<size_t> cols = {65, 80, 84, 85, 100, 128, 255, 256};
  size_t checked = 0;
  for (size_t D : cols)
    for (size_t n_r : refs)
      for (size_t n_b : batches) {
        size_t n_q = n_b;
        const WideReferenceLayout R = wide_reference_layout(n_r, D, n_b);
        const WideCrossPrunedLayout& P = R.P;
        const WideLayout& L = P.L;
        const size_t n_max = n_b > n_r ? n_b : n_r, tile_bytes = (size_t)16 * 64 * L.NM;
        CHECK(L.NM == (uint32_t)nm_for((int)D) && L.Tp % kWideBlockTiles == 0 && L.Tqp % kWideBlockTiles == 0);
        CHECK(P.blocks_r == (n_r + 127) / 128 && P.blocks_q == (n_b + 127) / 128);
        const Region resident[] = {{L.off_img_a, tile_bytes * L.Tp},    {L.off_norms, 4 * 32 * (size_t)L.Tp},
                                   {P.off_perm_r, 4 * n_r},             {P.off_coords_r, 4 * n_r * D},
                                   {P.off_boxes_r, 16 * (size_t)P.blocks_r}, {R.N.off_fe_r, 4 * n_r},
                                   {R.N.off_fe_min_r, 4 * (size_t)P.blocks_r}, {R.off_fe_row, 4 * n_r}};
        const Region batch[] = {{L.off_img_b, tile_bytes * L.Tqp},       {L.off_merge, 16 * n_b},
                                {P.off_perm_q, 4 * n_b},                 {P.off_coords_q, 4 * n_b * D},
                                {P.off_boxes_q, 16 * (size_t)P.blocks_q}, {P.off_cnt, 4 * (size_t)kMaxRadiiPerLaunch * n_b},
                                {R.N.off_fe_q, 4 * n_b},                 {R.N.off_qwords, 16 * (size_t)P.blocks_q}};
        const Region scratch[] = {{P.off_keys, 4 * n_max}, {P.off_keys_o, 4 * n_max}, {P.off_vals, 4 * n_max}, {P.off_sort, sort_temp_bytes(n_max)}};
        // the regions lie inside the total, in the order they are laid out, none over another; the header in front of all
        size_t end = kWideOffImages;
        CHECK(R.resident_begin == kWideOffImages);
        for (const Region& r : resident) {
          CHECK(r.off % 256 == 0 && r.off >= end && r.off + r.bytes <= R.resident_end);
          end = r.off + r.bytes;
        }
        // the resident and the batch regions do not overlap; the scratch lies behind both
        CHECK(R.resident_end <= R.batch_begin);
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
        CHECK(P.total % 256 == 0 && L.total == P.total && wide_reference_workspace_bytes(n_r, D, n_b) == P.total);
        CHECK(P.sort_bytes >= sort_temp_bytes(n_b) && P.sort_bytes >= sort_temp_bytes(n_r));
        // the header words of the resident form lie inside the header, clear of every other form's
        CHECK(4 * (kWideHdrResMref + 1) <= kHdrBytes && kWideHdrResFlagRef > kWideHdrOrderHash + 1 && R.N.off_flag_q == 4 * kWideHdrResFlagFeQuery);
        // every batch the handle takes: its images, words per block and counts fit where they are put, and the unit map is
        // the pruned cross sweep's of the same shape
        for (size_t q : {(size_t)1, n_b / 2 + 1, n_b}) {
          n_q = q;
          const uint32_t blocks_q = (uint32_t)((n_q + kWideBlockRows - 1) / kWideBlockRows);
          CHECK(wide_pad_tiles((uint32_t)((n_q + 31) / 32)) <= L.Tqp && blocks_q <= P.blocks_q);
          // the words per query block as nn_wide_cross_pruned forms their pointers: fe_max_q at off_qwords, far2 (nn, hd)
          // P.blocks_q words behind it and 2 P.blocks_q long, the seed behind that; a batch writes blocks_q words of each
          const size_t w_fe_max = R.N.off_qwords, w_far2 = w_fe_max + 4 * (size_t)P.blocks_q, w_seed = w_far2 + 4 * 2 * (size_t)P.blocks_q;
          CHECK(w_fe_max + 4 * (size_t)blocks_q <= w_far2 && w_far2 + 4 * ((size_t)P.blocks_q + blocks_q) <= w_seed);
          CHECK(w_seed + 4 * (size_t)blocks_q <= R.N.off_qwords + 16 * (size_t)P.blocks_q && w_seed + 4 * (size_t)blocks_q <= R.batch_end);
          // ... and of the reference: the least free energy per block, and the free energies by position and by row
          CHECK(R.N.off_fe_min_r + 4 * (size_t)P.blocks_r <= R.off_fe_row && R.N.off_fe_r + 4 * n_r <= R.N.off_fe_min_r);
          const WideCrossPrunedLayout C = wide_cross_pruned_layout(n_q, n_r, D);
          CHECK(C.L.Tp == L.Tp && C.L.NM == L.NM && C.blocks_r == P.blocks_r);
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
  // monotone in each argument; zero outside 65..256 columns and for a zero count
  for (size_t D : cols) {
    size_t n_r = 0, n_b = 0, n_q = 0;
    for (size_t fixed : {(size_t)1, (size_t)300, (size_t)20000}) {
      size_t last_r = 0, last_b = 0;
      for (size_t n : refs) {
        n_r = n, n_b = fixed;
        const size_t a = wide_reference_workspace_bytes(n, D, fixed), b = wide_reference_workspace_bytes(fixed, D, n);
        CHECK(a >= last_r && b >= last_b && a > 0 && b > 0);
        last_r = a, last_b = b;
      }
    }
    CHECK(wide_reference_workspace_bytes(0, D, 100) == 0 && wide_reference_workspace_bytes(100, D, 0) == 0);
  }
  for (size_t D : {(size_t)0, (size_t)1, (size_t)64, (size_t)257, (size_t)1000}) {
    size_t n_r = 1000, n_b = 1000, n_q = 0;
    CHECK(wide_reference_workspace_bytes(n_r, D, n_b) == 0);
  }
  std::printf("%s %zu layouts\n", fails ? "FAILED" : "ok", checked);
  return fails ? 1 : 0;
}
