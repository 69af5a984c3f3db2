// Host-side check of every byte range the radius-graph launchers and the neighbour-block launchers address in a workspace
// of 257..1024 columns (dc_mfma_wide.hip: launch_pairs_wide_mfma, launch_min_edge_wide_mfma, launch_pairs_wide_pruned,
// launch_min_edge_wide_pruned and the two forests' rounds of them; launch_nn_block_pack_wide, launch_nn_block_unpack_wide,
// wide_layout_status), built from the library's own layout functions -- wide_layout, wide_pruned_layout,
// nn_block_rows_of, the unit map -- and held to what the C API hands out: xwide_workspace_bytes and
// xwide_pruned_workspace_bytes.  Grid: rows 1 .. 70 000 x the column counts of the tests x segments 1, 2, 3, 5, 8.
// No device is touched: nothing here launches or allocates (tests/test_xwide_graph_layout.py runs it; it also builds
// under the host sanitizers, -Xarch_host -fsanitize=address,undefined).
#include <cstdio>
#include <vector>

#include "dc_mfma_wide.hip"

namespace dc {
void sweep_timer_mark(int, bool, hipStream_t) {}   // (dc_mfma.hip's, which this program does not link: nothing is launched here)
}  // namespace dc
using namespace dc;

static int fails = 0;
#define CHECK(c)                                                                              \
  do {                                                                                        \
    if (!(c)) {                                                                               \
      if (++fails <= 40) std::printf("FAILED %s (line %d) n=%zu D=%zu G=%zu\n", #c, __LINE__, n, D, G); \
    }                                                                                         \
  } while (0)

struct Region {
  size_t off, bytes;
};

int main() {
  const size_t cols[] = {257, 258, 261, 267, 272, 401, 512, 1024};
  const size_t segments[] = {1, 2, 3, 5, 8};
  const size_t kRowsMax = 70000;
  size_t checked = 0;
  for (size_t D : cols) {
    size_t last_plain = 0, last_pruned = 0;
    for (size_t n = 1; n <= kRowsMax; ++n) {
      size_t G = 0;
      const WideLayout L = wide_layout(n, D);
      const WidePrunedLayout P = wide_pruned_layout(n, D);
      const size_t plain = xwide_workspace_bytes(n, D), pruned = xwide_pruned_workspace_bytes(n, D);
      const size_t tile_bytes = (size_t)16 * 64 * L.NM, images = wide_off_images(D);
      // what the C API hands out is the layout the launchers read, and the 65..256 family's size functions are 0 here
      CHECK(plain == L.total && pruned == P.total && pruned >= plain && plain >= last_plain && pruned >= last_pruned);
      CHECK(wide_workspace_bytes(n, D) == 0 && wide_pruned_workspace_bytes(n, D) == 0);
      last_plain = plain, last_pruned = pruned;
      CHECK(L.NM == (uint32_t)nm_for((int)D) && L.NM >= 49 && L.NM <= 193 && L.Tp % kWideBlockTiles == 0 && L.Tq == L.T && L.Tqp == L.Tp);
      CHECK((size_t)L.Tp * 32 >= n && P.blocks == (n + kWideBlockRows - 1) / kWideBlockRows && P.blocks == L.Tp / kWideBlockTiles);
      // ---- the head: header words, sums [1024] doubles, means [1024] floats; the images start at byte 13 312 ----
      CHECK(images == 13312 && wide_off_means(D) == kWideOffSums + 8 * kXWideMaxCols && kWideOffSums == kHdrBytes);
      CHECK(wide_off_means(D) >= kWideOffSums + 8 * D && images >= wide_off_means(D) + 4 * D);
      const Region words[] = {{4 * kWideHdrTiles, 24},        // the three counters (wide_clear_counters, dc_hip_wide_info_dev)
                              {4 * kWideHdrExt, 16},          // the extent of columns 0 / 1
                              {4 * kWideHdrOrder, 12},        // the order's signature: mark, rows, columns
                              {4 * kWideHdrLayoutBad, 4},     // the verdict of the last unpack
                              {4 * kWideHdrOrderHash, 8},     // the hash of the order
                              {0, kWideInfoBytes}};           // what clear_wide_info clears
      for (const Region& w : words) CHECK(w.off + w.bytes <= kHdrBytes && w.off + w.bytes <= images && w.off + w.bytes <= plain);
      // ---- the unpruned launchers (wide_args of wide_layout): images, norms, merge words ----
      const Region head[] = {{L.off_img_a, tile_bytes * L.Tp}, {L.off_img_b, tile_bytes * L.Tqp}, {L.off_norms, 4 * 32 * (size_t)L.Tp},
                             {L.off_merge, 16 * n}};
      size_t end = images;
      for (const Region& r : head) {
        CHECK(r.off % 256 == 0 && r.off >= end && r.off >= images && r.off + r.bytes <= plain);
        end = r.off + r.bytes;
      }
      // the last fragment a workgroup fetches: tile Tp - 1, MFMA NM - 1, lane 63 (fetch(): ((t NM + m) 64 + lane) 16 bytes)
      CHECK((((size_t)(L.Tp - 1) * L.NM + (L.NM - 1)) * 64 + 63) * 16 + 16 == tile_bytes * L.Tp);
      // ---- the pruned launchers: the same head, then perm, keys, rows in the order, boxes, the count region, the sort ----
      CHECK(P.L.total == L.total && P.L.off_img_a == L.off_img_a && P.L.off_norms == L.off_norms && P.L.off_merge == L.off_merge);
      const Region tail[] = {{P.off_perm, 4 * n},
                             {P.off_keys, 4 * n},
                             {P.off_keys_o, 4 * n},
                             {P.off_vals, 4 * n},
                             {P.off_coords, 4 * n * D},
                             {P.off_boxes, 16 * (size_t)P.blocks},
                             {P.off_cnt, 4 * n},                          // row 0: the counts by position
                             {P.off_cnt + 4 * n, 4 * n},                  // row 1: comp gathered into the order
                             {P.off_cnt + 4 * 2 * n, 4 * n},              // row 2: rank gathered into the order
                             {P.off_sort, P.sort_bytes}};
      end = L.total;
      for (const Region& r : tail) {
        CHECK(r.off >= end && r.off >= images && r.off + r.bytes <= pruned);
        end = r.off + r.bytes;
      }
      CHECK(P.off_cnt + 4 * (size_t)kMaxRadiiPerLaunch * n <= P.off_sort && kMaxRadiiPerLaunch >= 3 && P.sort_bytes >= sort_temp_bytes(n));
      CHECK(P.off_perm % 256 == 0 && P.off_coords % 256 == 0 && P.off_boxes % 256 == 0 && P.off_cnt % 256 == 0 && P.off_sort % 256 == 0);
      // ---- the grids: every (query block, share) unit of a whole launch and of a segment's, each once, none beyond ----
      const uint32_t shares = wide_shares(P.blocks);
      CHECK(shares >= 1 && shares <= kWideShares && (shares == 1 || shares * kWideShareBlocks <= P.blocks));
      const bool deep = n <= 1300 || n % 4999 == 0 || n == kRowsMax;   // (the unit maps: a sample of the rows)
      for (size_t g_count : segments) {
        G = g_count;
        // the blocks: rows of a block, the payload, the header words at its end, the largest local position of either mode
        const size_t rows = nn_block_rows_of(n, G), payload = rows - kWideBlockHdrRows;
        CHECK(rows == xwide_nn_block_rows(n, D, G) && wide_nn_block_rows(n, D, G) == 0 && rows > kWideBlockHdrRows && rows <= 0xFFFFFFFFull);
        CHECK(kWideBlockHdrWords <= kWideBlockHdrRows && payload + kWideBlockHdrWords <= rows);
        const size_t rng = n / G, last_block = n - (G - 1) * rng;
        CHECK(last_block <= payload && rng <= payload);                       // row blocks: l = p - r rng < payload
        CHECK(((P.blocks - 1) / G) * kWideBlockRows + kWideBlockRows - 1 < payload);   // by position: l of the last block's last position
        for (size_t seg = 0; seg < G; ++seg) {
          // pack: the positions p(l) of the payload that are read from perm lie below n (the kernel's guard) or are pads
          const size_t owned = seg < P.blocks ? (P.blocks - seg + G - 1) / G : 0;
          CHECK(owned * kWideBlockRows <= payload);
          if (owned) CHECK(((owned - 1) * G + seg) < P.blocks);
          if (!deep || seg >= P.blocks) continue;
          const uint32_t q_blocks = (uint32_t)owned, grid = wide_grid_size(q_blocks, shares);
          CHECK(grid % 512 == 0 && grid >= q_blocks * shares);
          std::vector<char> seen((size_t)q_blocks * shares, 0);
          for (uint32_t id = 0; id < grid; ++id) {
            const WideUnit u = wide_unit(id, shares);
            CHECK(u.share < shares);
            const unsigned long long q = seg + (unsigned long long)u.q_block * G;   // (the kernel's own guard: q >= RB returns)
            if (q >= P.blocks) continue;
            CHECK(u.q_block < q_blocks && !seen[(size_t)u.q_block * shares + u.share]);
            if (u.q_block < q_blocks) seen[(size_t)u.q_block * shares + u.share] = 1;
          }
          for (char c : seen) CHECK(c == 1);
        }
        ++checked;
      }
    }
  }
  // outside the family: no bytes, no block rows
  for (size_t D : {(size_t)0, (size_t)64, (size_t)65, (size_t)256, (size_t)1025}) {
    const size_t n = 1000, G = 3;
    CHECK(xwide_workspace_bytes(n, D) == 0 && xwide_pruned_workspace_bytes(n, D) == 0 && xwide_nn_block_rows(n, D, G) == 0);
  }
  {
    const size_t n = 0, D = 300, G = 0;
    CHECK(xwide_workspace_bytes(0, D) == 0 && xwide_pruned_workspace_bytes(0, D) == 0 && xwide_nn_block_rows(0, D, 3) == 0 &&
          xwide_nn_block_rows(10, D, 0) == 0);
  }
  std::printf("%s %zu layouts\n", fails ? "FAILED" : "ok", checked);
  return fails ? 1 : 0;
}
