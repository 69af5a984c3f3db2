// Host-side check of the workspace arithmetic of the resident reference for rows of 1..64 columns
// (clustering_amd/csrc/dc_reference_layout.hpp) under the host sanitizers.  No device is touched: nothing here launches
// or allocates.
//   cd clustering_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I. -I../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -o /tmp/reference_layout_check ../../scratch/reference_layout_check.hip dc_sort.hip && /tmp/reference_layout_check
#include <cstdio>
#include <vector>

#include "dc_mfma_kernels.hpp"

namespace dc {
namespace {
#include "dc_reference_layout.hpp"
}
}  // namespace dc
using namespace dc;

static int fails = 0;
#define CHECK(c)                                                                                  \
  do {                                                                                            \
    if (!(c)) {                                                                                   \
      ++fails;                                                                                    \
      std::printf("FAILED %s (line %d) n_r=%zu D=%zu max_batch=%zu\n", #c, __LINE__, n_r, D, n_b); \
    }                                                                                             \
  } while (0)

struct Region {
  size_t off, bytes;
};

int main() {
  const std::vector<size_t> refs = {1, 2, 31, 32, 33, 1000, 1500, 8320, 57600, 1000000, ((size_t)1 << 24) - 31, (size_t)1 << 24};
  const std::vector<size_t> batches = {1, 31, 32, 33, 191, 192, 193, 300, 1100, 100000, 2000000};
  const std::vector<size_t> cols = {1, 2, 3, 4, 5, 7, 10, 16, 24, 30, 31, 32, 33, 63, 64};
  size_t checked = 0;
  for (size_t D : cols)
    for (size_t n_r : refs)
      for (size_t n_b : batches) {
        const ReferenceLayout R = reference_layout(n_r, D, n_b);
        const size_t n_max = n_b > n_r ? n_b : n_r, tile_bytes = (size_t)16 * 64 * R.NM;
        const size_t pos_r = (size_t)32 * R.T_r, pos_q = (size_t)32 * R.T_q;
        CHECK(R.NM == (uint32_t)nm_for((int)D) && R.T_r == (n_r + 31) / 32 && R.T_q == (n_b + 31) / 32);
        std::vector<Region> resident, batch;
        for (const ReferenceSide* S : {&R.pop, &R.nn}) {
          resident.insert(resident.end(), {{S->off_img_r, tile_bytes * R.T_r}, {S->off_norm_r, 4 * pos_r}, {S->off_perm_r, 4 * pos_r},
                                           {S->off_coords_r, 4 * pos_r * D}, {S->off_box_r, 16 * (size_t)R.T_r}});
          batch.insert(batch.end(), {{S->off_img_q, tile_bytes * R.T_q}, {S->off_norm_q, 4 * pos_q}, {S->off_perm_q, 4 * pos_q},
                                     {S->off_box_q, 16 * (size_t)R.T_q}});
        }
        // (laid out side by side: the population side's arrays of R, then the neighbour side's, then the free-energy words)
        resident.insert(resident.end(), {{R.off_fe_c, 4 * pos_r}, {R.off_ferange, 8 * (size_t)R.T_r}, {R.off_meta, 5 * 4}, {R.off_fe_row, 4 * n_r},
                                         {R.off_fe_c_none, 4 * pos_r}, {R.off_ferange_none, 8 * (size_t)R.T_r}});
        batch.insert(batch.end(), {{R.off_merge64, 16 * pos_q}, {R.off_keys_nn, 4 * n_b}, {R.off_vals_nn, 4 * n_b}});
        const Region scratch[] = {{R.off_keys_in, 4 * n_max}, {R.off_keys_out, 4 * n_max}, {R.off_vals_in, 4 * n_max}, {R.off_sort, sort_temp_bytes(n_max)}};
        // the header and the resident words in front of everything; the regions inside the total, in the order they are
        // laid out, none over another
        CHECK(R.resident_begin == kHdrBytes + kRefWordsBytes && kRefOffArrays % 256 == 0);
        size_t end = R.resident_begin;
        for (const Region& r : resident) {
          CHECK(r.off % 256 == 0 && r.off >= end && r.off + r.bytes <= R.resident_end);
          end = r.off + r.bytes;
        }
        CHECK(R.resident_end <= R.batch_begin);
        end = R.batch_begin;
        for (const Region& r : batch) {
          CHECK(r.off % 256 == 0 && r.off >= end && r.off + r.bytes <= R.batch_end);
          end = r.off + r.bytes;
        }
        end = R.batch_end;
        for (const Region& r : scratch) {
          CHECK(r.off % 256 == 0 && r.off >= end && r.off + r.bytes <= R.total);
          end = r.off + r.bytes;
        }
        CHECK(R.total % 256 == 0 && R.sort_bytes >= sort_temp_bytes(n_b) && R.sort_bytes >= sort_temp_bytes(n_r));
        // every batch the handle takes: what a stage and the sweeps write fits where it is put
        for (size_t n_q : {(size_t)1, n_b / 2 + 1, n_b}) {
          const size_t T_q = (n_q + 31) / 32;
          CHECK(T_q <= R.T_q && 32 * T_q <= pos_q && n_q <= n_max);
          CHECK(R.nn.off_img_q + tile_bytes * T_q <= R.nn.off_norm_q && R.off_merge64 + 16 * 32 * T_q <= R.off_keys_nn);
          ++checked;
        }
      }
  // monotone in each argument; sizes for a zero count are the caller's to refuse (reference_workspace_bytes returns 0)
  for (size_t D : cols) {
    size_t n_r = 0, n_b = 0;
    for (size_t fixed : {(size_t)1, (size_t)300, (size_t)100000}) {
      size_t last_r = 0, last_b = 0;
      for (size_t n : refs) {
        n_r = n, n_b = fixed;
        const size_t a = reference_layout(n, D, fixed).total, b = reference_layout(fixed, D, n).total;
        CHECK(a >= last_r && b >= last_b && a > 0 && b > 0);
        last_r = a, last_b = b;
      }
    }
  }
  std::printf("%s %zu layouts\n", fails ? "FAILED" : "ok", checked);
  return fails ? 1 : 0;
}
