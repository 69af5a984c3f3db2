// Host check of the placement of the per-wave pruned sweeps' units (clustering_amd/csrc/dc_sweep_units.hpp).  For every
// n_blocks in {1, 7, 8, 9, 63, 64, 65, 659, 5209} and n_chunks in {1, 2, 7, 8, 10, 64}:
//   * the decode over all (queue, ticket < length) is a bijection onto (block unit < n_blocks, share < n_chunks);
//   * the queue lengths sum to n_blocks * n_chunks, and the tickets from the length on decode to "no unit";
//   * queue q's sequence is what the static form gives the blocks with x & 7 == q, in the order they are started
//     (x fastest, then y), pad blocks left out.
// Prints "ok <units checked>" and returns 0, or the first violations and 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dc_sweep_units.hpp"

int main() {
  const uint32_t blocks[] = {1, 7, 8, 9, 63, 64, 65, 659, 5209}, chunks[] = {1, 2, 7, 8, 10, 64};
  long checked = 0;
  int failures = 0;
  auto fail = [&](const char* what, uint32_t nb, uint32_t nc, uint32_t q, uint32_t t) {
    if (++failures <= 10) std::printf("FAIL %s: n_blocks=%u n_chunks=%u queue=%u ticket=%u\n", what, nb, nc, q, t);
  };
  for (uint32_t nb : blocks)
    for (uint32_t nc : chunks) {
      std::vector<uint32_t> seen((size_t)nb * nc, 0u);
      unsigned long long total = 0;
      for (uint32_t q = 0; q < kSweepQueues; ++q) {
        const uint32_t len = sweep_queue_len(nb, nc, q);
        total += len;
        // the static form's sequence of this label: y outermost, then the blocks x = q, q + 8, ... of the padded grid
        uint32_t ticket = 0;
        const uint32_t grid_x = (nb + 7u) & ~7u;
        for (uint32_t y = 0; y < nc; ++y)
          for (uint32_t x = q; x < grid_x; x += 8) {
            const uint32_t blk = xcd_unit(nb, x, y);
            if (blk == kNoUnit) continue;
            const SweepUnit u = sweep_unit(nb, nc, q, ticket);
            if (u.blk != blk || u.share != y) fail("the queue is not the static sequence", nb, nc, q, ticket);
            if (u.blk < nb && u.share < nc)
              ++seen[(size_t)u.share * nb + u.blk];
            else
              fail("unit out of range", nb, nc, q, ticket);
            ++ticket;
            ++checked;
          }
        if (ticket != len) fail("queue length", nb, nc, q, ticket);
        // past the end: the overshoot of every workgroup that finds the queue empty, and far beyond
        for (uint32_t t : {len, len + 1u, len + 2048u, 0x7FFFFFFFu, 0xFFFFFFFFu})
          if (sweep_unit(nb, nc, q, t).blk != kNoUnit) fail("a ticket past the end decodes to a unit", nb, nc, q, t);
      }
      if (total != (unsigned long long)nb * nc) fail("the lengths do not sum to the units", nb, nc, 0, 0);
      for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1u) {
          fail("a unit is drawn never or twice", nb, nc, (uint32_t)(i / nb), (uint32_t)(i % nb));
          break;
        }
    }
  if (sweep_unit(0, 4, 0, 0).blk != kNoUnit || sweep_queue_len(0, 4, 3) != 0) fail("no blocks", 0, 4, 0, 0);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok %ld\n", checked);
  return 0;
}
