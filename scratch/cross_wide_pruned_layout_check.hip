// Host-side check of the pruned wide cross sweep's workspace arithmetic (dc_mfma_wide.hip wide_cross_pruned_layout,
// wide_cross_pruned_workspace_bytes) under the host sanitizers.  No device is touched: nothing here launches or allocates.
//   cd clustering_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I. -I../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -o /tmp/cross_wide_pruned_layout_check ../../scratch/cross_wide_pruned_layout_check.hip dc_sort.hip && /tmp/cross_wide_pruned_layout_check
#include <cstdio>
#include <vector>

#include "dc_mfma_wide.hip"

namespace dc {
void sweep_timer_mark(int, bool, hipStream_t) {}   // (dc_mfma.hip's, which this program does not link: nothing is launched here)
}  // namespace dc
using namespace dc;

static int fails = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      ++fails;                                                            \
      std::printf("FAILED %s (line %d) n_q=%zu n_r=%zu D=%zu\n", #c, __LINE__, n_q, n_r, D); \
    }                                                                     \
  } while (0)

int main() {
  const std::vector<size_t> sizes = {1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000, 1001, 4096, 8320, 20000, 100000, 200000, 1000000, 4000000};
  const std::vector<size_t> cols = {65, 80, 84, 85, 100, 127, 128, 129, 255, 256};
  size_t checked = 0;
  for (size_t D : cols)
    for (size_t n_q : sizes)
      for (size_t n_r : sizes) {
        const WideCrossPrunedLayout P = wide_cross_pruned_layout(n_q, n_r, D);
        const WideLayout L = wide_layout_against(n_q, n_r, D);
        const size_t n_max = n_q > n_r ? n_q : n_r;
        // regions in the order they are laid out: (offset, bytes)
        const std::pair<size_t, size_t> reg[] = {
            {0, L.total},
            {P.off_perm_r, 4 * n_r},
            {P.off_perm_q, 4 * n_q},
            {P.off_keys, 4 * n_max},
            {P.off_keys_o, 4 * n_max},
            {P.off_vals, 4 * n_max},
            {P.off_coords_r, 4 * n_r * D},
            {P.off_coords_q, 4 * n_q * D},
            {P.off_boxes_r, 16 * (size_t)P.blocks_r},
            {P.off_boxes_q, 16 * (size_t)P.blocks_q},
            {P.off_cnt, 4 * (size_t)kMaxRadiiPerLaunch * n_q},
            {P.off_sort, sort_temp_bytes(n_max)},
        };
        size_t end = 0;
        for (const auto& r : reg) {
          CHECK(r.first % 256 == 0);
          CHECK(r.first >= end);
          end = r.first + r.second;
        }
        CHECK(P.total >= end && P.total % 256 == 0);
        CHECK(P.blocks_r == (n_r + 127) / 128 && P.blocks_q == (n_q + 127) / 128);
        CHECK(P.sort_bytes >= sort_temp_bytes(n_q) && P.sort_bytes >= sort_temp_bytes(n_r));
        CHECK(wide_cross_pruned_workspace_bytes(n_q, n_r, D) == P.total);
        CHECK(P.total >= wide_against_workspace_bytes(n_q, n_r, D));
        // the head is the unpruned cross sweeps': dc_hip_wide_info_dev and the kernels read the same words
        CHECK(P.L.off_img_a == L.off_img_a && P.L.off_img_b == L.off_img_b && P.L.off_norms == L.off_norms && P.L.Tp == L.Tp);
        // the B image of a gathered range of the queries fits the region laid out for all of them
        for (size_t n_range : {(size_t)1, n_q / 2 + 1, n_q})
          CHECK(wide_pad_tiles((uint32_t)((n_range + 31) / 32)) <= L.Tqp);
        // the launch: one workgroup group per 8 x 64 / shares query blocks, every query block inside the grid
        const uint32_t shares = wide_shares(P.blocks_r), grid = wide_grid_size(P.blocks_q, shares);
        CHECK(shares >= 1 && shares <= kWideShares && grid % 512 == 0);
        std::vector<char> seen((size_t)P.blocks_q * shares, 0);
        if (P.blocks_q <= 64) {
          for (uint32_t id = 0; id < grid; ++id) {
            const WideUnit u = wide_unit(id, shares);
            CHECK(u.share < shares);
            if (u.q_block < P.blocks_q) {
              CHECK(!seen[(size_t)u.q_block * shares + u.share]);
              seen[(size_t)u.q_block * shares + u.share] = 1;
            }
          }
          for (char c : seen) CHECK(c == 1);
        }
        ++checked;
      }
  // monotone in either count; zero outside 65..256 columns and for an empty side
  for (size_t D : cols) {
    size_t n_q = 0, n_r = 0;
    for (size_t fixed : {(size_t)1, (size_t)300, (size_t)20000}) {
      size_t last_q = 0, last_r = 0;
      for (size_t n : sizes) {
        n_q = n, n_r = fixed;
        const size_t a = wide_cross_pruned_workspace_bytes(n, fixed, D), b = wide_cross_pruned_workspace_bytes(fixed, n, D);
        CHECK(a >= last_q && b >= last_r && a > 0 && b > 0);
        last_q = a, last_r = b;
      }
    }
    n_q = 0, n_r = 100;
    CHECK(wide_cross_pruned_workspace_bytes(0, 100, D) == 0 && wide_cross_pruned_workspace_bytes(100, 0, D) == 0);
  }
  for (size_t D : {(size_t)0, (size_t)1, (size_t)64, (size_t)257, (size_t)1000}) {
    size_t n_q = 1000, n_r = 1000;
    CHECK(wide_cross_pruned_workspace_bytes(n_q, n_r, D) == 0);
  }
  std::printf("%s %zu layouts\n", fails ? "FAILED" : "ok", checked);
  return fails ? 1 : 0;
}
