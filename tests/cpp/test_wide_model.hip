// test_wide_model.hip -- the chain of the wide matrix-core sweeps (65..256 columns) end to end against its band.
//
//   test_wide_model               GPU: for D = 65, 128, 256 and data scales 1e-3 .. 1e3, clustered frames go through the
//                                 product's own preparation (statistics, pick_scale_nn, operand images) and through
//                                 wide_sweep_kernel in its dump mode, which stores the accumulator of every pair instead
//                                 of classifying it.  Asserts  | acc - S d2 | <= e0 + kappa S d2  for every pair (d2 in
//                                 double from the original coordinates; the canonical float sum lies within the band's own
//                                 (D/4 + 9) u d2 of it), the self pairs and the duplicate rows included, and prints the
//                                 worst ratio |error| / band.  Exit 0 when all hold, 1 otherwise.
//   test_wide_model --band D M    host only (no device is touched): the scale and band the sweeps use for D columns
//                                 and max |x - mean|^2 = M, as "band D S e0 kappa" (e0 in scaled units) -- what the
//                                 case generators of tests/wideref.py measure their data with.
//   test_wide_model --shares RB   host only: "shares RB S", S = wide_shares(RB), the reference shares of a sweep over RB
//                                 reference blocks of 128 rows.
//   test_wide_model --units S QB  host only: "grid G", G = wide_grid_size(QB, S), then one line "id q_block share" per
//                                 workgroup id 0 .. G - 1 as wide_unit(id, S) decodes it (tests/test_wide_big_cases.py
//                                 checks that every query block meets every share exactly once).
// Built by clustering_amd/csrc/Makefile, run by tests/test_gpu_wide_model.py, tests/test_wide_mfma_cases.py and
// tests/test_wide_big_cases.py.
#include "../../clustering_amd/csrc/dc_mfma_wide_kernels.hpp"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace dc;

#define CHECK(x)                                                     \
  do {                                                               \
    hipError_t e_ = (x);                                             \
    if (e_ != hipSuccess) {                                          \
      fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_)); \
      return 2;                                                      \
    }                                                                \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double urand() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) / 9007199254740992.0;
}
static double nrand() { return sqrt(-2.0 * log(urand() + 1e-300)) * cos(6.283185307179586 * urand()); }

static int run_case(int D, double scale, double* worst_out) {
  const uint32_t n = 250;   // two blocks of 128 rows, the second partial
  std::vector<float> x((size_t)n * D);
  // four clusters of width 0.1 whose centres lie ~1 apart, offset from the origin; rows 7 and 8 are duplicates
  std::vector<double> centre(4 * (size_t)D);
  for (auto& c : centre) c = 3.0 + nrand() * (1.0 / sqrt((double)D));
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < D; ++k) x[(size_t)i * D + k] = (float)(scale * (centre[(i % 4) * (size_t)D + k] + 0.1 * nrand() / sqrt((double)D)));
  for (int k = 0; k < D; ++k) x[(size_t)8 * D + k] = x[(size_t)7 * D + k];

  const WideLayout L = wide_layout(n, (size_t)D);
  float* d_x = nullptr;
  char* d_ws = nullptr;
  float* d_dump = nullptr;
  const size_t np = (size_t)32 * L.Tp;
  CHECK(hipMalloc(&d_x, x.size() * sizeof(float)));
  CHECK(hipMalloc(&d_ws, L.total));
  CHECK(hipMalloc(&d_dump, np * np * sizeof(float)));
  CHECK(hipMemcpy(d_x, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice));
  if (wide_prepare_launches(d_x, n, (uint32_t)D, nullptr, d_ws, nullptr) != 0) return 2;
  WideArgs X{};
  X.coords = d_x;
  X.n_rows = n;
  X.n_cols = (uint32_t)D;
  X.NM = L.NM;
  X.Tp = L.Tp;
  X.img_a = (const uint4*)(d_ws + L.off_img_a);
  X.img_b = (const uint4*)(d_ws + L.off_img_b);
  X.norms = (const float*)(d_ws + L.off_norms);
  X.hdr = (uint32_t*)d_ws;
  X.i_from = 0;
  X.i_to = n;
  X.dump = d_dump;
  hipLaunchKernelGGL((wide_sweep_kernel<kWideDump, 1>), dim3(wide_grid_size(L.Tp / kWideBlockTiles, wide_shares(L.Tp / kWideBlockTiles))), dim3(256), 0, nullptr, X);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<float> acc(np * np);
  uint32_t hdr[64];
  CHECK(hipMemcpy(acc.data(), d_dump, acc.size() * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hdr, d_ws, sizeof(hdr), hipMemcpyDeviceToHost));
  CHECK(hipFree(d_x));
  CHECK(hipFree(d_ws));
  CHECK(hipFree(d_dump));
  if (hdr[1] != 0) {
    printf("D=%d scale=%g: the data was flagged\n", D, scale);
    return 1;
  }
  ScaleExp se;
  se.c = __builtin_bit_cast(float, hdr[kHdrScale]);
  se.s2 = __builtin_bit_cast(float, hdr[kHdrScale + 1]);
  se.g = (int)hdr[kHdrScale + 2];
  se.a = (int)hdr[kHdrScale + 3];
  se.rounded = (int)hdr[kHdrScale + 4];
  const Scale sc = make_scale(se);
  const float M = __builtin_bit_cast(float, hdr[0]);
  const WideBand b = wide_band(M * sc.s2, D, sc);
  double worst = 0.0;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < n; ++j) {
      double d2 = 0.0;
      for (int k = 0; k < D; ++k) {
        const double c = (double)x[(size_t)i * D + k] - (double)x[(size_t)j * D + k];
        d2 += c * c;
      }
      const double sd2 = d2 * (double)sc.s2, err = fabs((double)acc[(size_t)i * np + j] - sd2);
      const double ratio = err / ((double)b.e0 + (double)b.kappa * sd2);
      if (!(ratio <= worst)) worst = ratio;   // (a NaN accumulator ends up here too)
    }
  // pad rows: +inf through the reference norm
  for (uint32_t i = n; i < np; ++i)
    if (!(acc[(size_t)i * np + 0] == INFINITY)) {
      printf("D=%d scale=%g: pad reference row %u is not +inf\n", D, scale, i);
      return 1;
    }
  printf("D=%3d NM=%2u scale=%-6g S=2^%d M*S=%.4g e0=%.4g kappa=%.3g worst |err|/band = %.4f\n", D, L.NM, scale,
         (int)lrint(log2((double)sc.s2)), (double)M * sc.s2, (double)b.e0, (double)b.kappa, worst);
  *worst_out = worst;
  return (worst <= 1.0) ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "--band") == 0) {
    const int D = atoi(argv[2]);
    const float M = (float)atof(argv[3]);
    const ScaleExp se = pick_scale_nn(M);
    const Scale sc = make_scale(se);
    const WideBand b = wide_band(M * sc.s2, D, sc);
    printf("band %d %.9g %.9g %.9g\n", D, (double)sc.s2, (double)b.e0, (double)b.kappa);
    return 0;
  }
  if (argc == 3 && strcmp(argv[1], "--shares") == 0) {
    const uint32_t rb = (uint32_t)strtoul(argv[2], nullptr, 10);
    printf("shares %u %u\n", rb, wide_shares(rb));
    return 0;
  }
  if (argc == 4 && strcmp(argv[1], "--units") == 0) {
    const uint32_t n_shares = (uint32_t)strtoul(argv[2], nullptr, 10), q_blocks = (uint32_t)strtoul(argv[3], nullptr, 10);
    if (n_shares == 0 || n_shares > kWideShares || (n_shares & (n_shares - 1u)) != 0) {
      fprintf(stderr, "--units: the shares are a power of two up to %u\n", kWideShares);
      return 2;
    }
    const uint32_t grid = wide_grid_size(q_blocks, n_shares);
    printf("grid %u\n", grid);
    for (uint32_t id = 0; id < grid; ++id) {
      const WideUnit u = wide_unit(id, n_shares);
      printf("%u %u %u\n", id, u.q_block, u.share);
    }
    return 0;
  }
  int bad = 0;
  double worst_all = 0.0;
  for (int D : {65, 128, 256})
    for (double scale : {1e-3, 1.0, 1e3}) {
      double w = 0.0;
      const int rc = run_case(D, scale, &w);
      if (rc == 2) return 2;
      bad |= rc;
      if (w > worst_all) worst_all = w;
    }
  printf("worst ratio over all cases: %.4f\n", worst_all);
  printf(bad ? "FAILED\n" : "OK\n");
  return bad;
}
