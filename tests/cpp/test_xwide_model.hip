// test_xwide_model.hip -- the chain of the matrix-core sweeps at 257..1024 columns end to end.
//
//   test_xwide_model              GPU.  Three checks, each printed; exit 0 when all hold, 1 otherwise.
//     band    D = 257, 512, 1024 at data scales 1e-3, 1, 1e3: clustered frames go through the product's own preparation
//             (statistics, pick_scale_nn, operand images in the layout of these widths) and through wide_sweep_kernel in
//             its dump mode.  Asserts | acc - S d2 | <= e0 + kappa S d2 for every pair (d2 in double from the original
//             coordinates), duplicates and self pairs included, and prints the worst |error| / band per case.
//     means   D = 1024, every column centred far from 0: after the preparation every one of the D means in the workspace
//             equals the float64 column mean within 4 ulp of the largest |value| of the column.  No result depends on the
//             means -- any origin serves, the band covers it --, so a column the statistics leave at 0 can only be seen here.
//     chunks  D = 257, 261, 267, 272 (NM = 49, 50, 51, 52: every NM mod 4): the accumulators of the sweep, whose chain runs
//             in LDS chunks of kWideKC MFMAs with a short last chunk, equal bit for bit those of a model that runs the same
//             chain ONE MFMA at a time straight from the operand images -- a chunk of one, so no last-chunk rule to get
//             wrong.  (The model issues its MFMAs on the device: how the instruction truncates and rounds is the
//             hardware's, tests/cpp/test_mfma_model.hip.)
//   test_xwide_model --band D M   host only: "band D S e0 kappa" as tests/cpp/test_wide_model.hip prints it.
//   test_xwide_model --units GQ GS RB QB   host only: the unit map of a GQ x GS group (wide_shares, wide_grid_size, wide_unit).
// Built by clustering_amd/csrc/Makefile, run by tests/test_gpu_xwide_model.py.
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

// the chain of tile pair (reference tile blockIdx.x, query tile blockIdx.y), one MFMA at a time from the images: one wave
__global__ __launch_bounds__(64) void chain_model_kernel(const uint4* __restrict__ img_a, const uint4* __restrict__ img_b,
                                                         const float* __restrict__ norms, uint32_t NM, uint32_t Tp,
                                                         float* __restrict__ dump) {
  const uint32_t lane = threadIdx.x, h = lane >> 5, c = lane & 31u, rt = blockIdx.x, qt = blockIdx.y;
  float4 nv[4];
  load_frag(norms, rt, (int)h, nv);
  f32x16 acc = frag16(nv);
  const u32x4* a = reinterpret_cast<const u32x4*>(img_a);
  const u32x4* b = reinterpret_cast<const u32x4*>(img_b);
  for (uint32_t m = 0; m < NM; ++m)
    acc = mfma16(__builtin_bit_cast(s16x8, a[((size_t)rt * NM + m) * 64 + lane]),
                 __builtin_bit_cast(s16x8, b[((size_t)qt * NM + m) * 64 + lane]), acc);
#pragma unroll
  for (int g = 0; g < 16; ++g)
    dump[(size_t)(rt * 32u + tile_row_local(g, (int)h)) * (32u * Tp) + qt * 32u + c] = acc[g];
}

struct Case {
  std::vector<float> x;        // [n][D]
  std::vector<float> acc;      // [np][np] of the sweep
  std::vector<float> model;    // [np][np] of the one-MFMA-at-a-time model (filled on request)
  std::vector<float> means;    // [D] as the workspace holds them
  uint32_t hdr[64];
  uint32_t n, np, NM;
};

// four clusters of width 0.1 whose centres lie ~1 apart around (3, 3, ..); rows 7 and 8 are duplicates
static void make_rows(uint32_t n, int D, double scale, std::vector<float>* x) {
  x->resize((size_t)n * D);
  std::vector<double> centre(4 * (size_t)D);
  for (auto& c : centre) c = 3.0 + nrand() * (1.0 / sqrt((double)D));
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < D; ++k) (*x)[(size_t)i * D + k] = (float)(scale * (centre[(i % 4) * (size_t)D + k] + 0.1 * nrand() / sqrt((double)D)));
  for (int k = 0; k < D; ++k) (*x)[(size_t)8 * D + k] = (*x)[(size_t)7 * D + k];
}

static int run_device(int D, bool with_model, Case* cs) {
  const uint32_t n = cs->n;
  const WideLayout L = wide_layout(n, (size_t)D);
  float* d_x = nullptr;
  char* d_ws = nullptr;
  float* d_dump = nullptr;
  const size_t np = (size_t)32 * L.Tp;
  cs->np = (uint32_t)np;
  cs->NM = L.NM;
  CHECK(hipMalloc(&d_x, cs->x.size() * sizeof(float)));
  CHECK(hipMalloc(&d_ws, L.total));
  CHECK(hipMalloc(&d_dump, np * np * sizeof(float)));
  CHECK(hipMemcpy(d_x, cs->x.data(), cs->x.size() * sizeof(float), hipMemcpyHostToDevice));
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
  hipLaunchKernelGGL((wide_sweep_kernel<kWideDump, 1>), dim3(wide_grid_size(L.Tp / kWideBlockTiles, wide_shares(L.Tp / kWideBlockTiles))),
                     dim3(256), 0, nullptr, X);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  cs->acc.resize(np * np);
  cs->means.resize((size_t)D);
  CHECK(hipMemcpy(cs->acc.data(), d_dump, cs->acc.size() * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(cs->hdr, d_ws, sizeof(cs->hdr), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(cs->means.data(), d_ws + wide_off_means((size_t)D), sizeof(float) * (size_t)D, hipMemcpyDeviceToHost));
  if (with_model) {
    CHECK(hipMemset(d_dump, 0, np * np * sizeof(float)));
    hipLaunchKernelGGL(chain_model_kernel, dim3(L.Tp, L.Tp), dim3(64), 0, nullptr, X.img_a, X.img_b, X.norms, L.NM, L.Tp, d_dump);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    cs->model.resize(np * np);
    CHECK(hipMemcpy(cs->model.data(), d_dump, cs->model.size() * sizeof(float), hipMemcpyDeviceToHost));
  }
  CHECK(hipFree(d_x));
  CHECK(hipFree(d_ws));
  CHECK(hipFree(d_dump));
  return 0;
}

static int band_case(int D, double scale, double* worst_out) {
  Case cs;
  cs.n = 250;   // two blocks of 128 rows, the second partial
  make_rows(cs.n, D, scale, &cs.x);
  if (int rc = run_device(D, false, &cs)) return rc;
  if (cs.hdr[1] != 0) {
    printf("D=%d scale=%g: the data was flagged\n", D, scale);
    return 1;
  }
  ScaleExp se;
  se.c = __builtin_bit_cast(float, cs.hdr[kHdrScale]);
  se.s2 = __builtin_bit_cast(float, cs.hdr[kHdrScale + 1]);
  se.g = (int)cs.hdr[kHdrScale + 2];
  se.a = (int)cs.hdr[kHdrScale + 3];
  se.rounded = (int)cs.hdr[kHdrScale + 4];
  const Scale sc = make_scale(se);
  const float M = __builtin_bit_cast(float, cs.hdr[0]);
  const WideBand b = wide_band(M * sc.s2, D, sc);
  const uint32_t n = cs.n, np = cs.np;
  double worst = 0.0;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < n; ++j) {
      double d2 = 0.0;
      for (int k = 0; k < D; ++k) {
        const double c = (double)cs.x[(size_t)i * D + k] - (double)cs.x[(size_t)j * D + k];
        d2 += c * c;
      }
      const double sd2 = d2 * (double)sc.s2, err = fabs((double)cs.acc[(size_t)i * np + j] - sd2);
      const double ratio = err / ((double)b.e0 + (double)b.kappa * sd2);
      if (!(ratio <= worst)) worst = ratio;   // (a NaN accumulator ends up here too)
    }
  for (uint32_t i = n; i < np; ++i)
    if (!(cs.acc[(size_t)i * np + 0] == INFINITY)) {
      printf("D=%d scale=%g: pad reference row %u is not +inf\n", D, scale, i);
      return 1;
    }
  printf("D=%4d NM=%3u scale=%-6g S=2^%d M*S=%.4g e0=%.4g kappa=%.3g worst |err|/band = %.4f\n", D, cs.NM, scale,
         (int)lrint(log2((double)sc.s2)), (double)M * sc.s2, (double)b.e0, (double)b.kappa, worst);
  *worst_out = worst;
  return (worst <= 1.0) ? 0 : 1;
}

static int means_case() {
  const int D = (int)kXWideMaxCols;
  Case cs;
  cs.n = 250;
  make_rows(cs.n, D, 1.0, &cs.x);
  // columns >= 256 further out still, each by its own amount and with either sign
  for (uint32_t i = 0; i < cs.n; ++i)
    for (int k = 256; k < D; ++k) cs.x[(size_t)i * D + k] += (float)(((k & 1) ? -1.0 : 1.0) * (5.0 + 0.01 * k));
  if (int rc = run_device(D, false, &cs)) return rc;
  int bad = 0;
  double worst_ulps = 0.0, least_abs_mean = INFINITY;
  for (int k = 0; k < D; ++k) {
    double sum = 0.0, big = 0.0;
    for (uint32_t i = 0; i < cs.n; ++i) {
      sum += (double)cs.x[(size_t)i * D + k];
      big = fmax(big, fabs((double)cs.x[(size_t)i * D + k]));
    }
    const double mean = sum / cs.n;
    int e = 0;
    (void)frexp(big, &e);                         // big = f 2^e, f in [0.5, 1): the floats at |big| are 2^(e - 24) apart
    const double ulp = ldexp(1.0, e - 24), off = fabs((double)cs.means[(size_t)k] - mean) / ulp;
    worst_ulps = fmax(worst_ulps, off);
    least_abs_mean = fmin(least_abs_mean, fabs(mean));
    if (!(off <= 4.0)) {
      if (bad < 5) printf("means: column %d holds %.9g, the column mean is %.17g (%.3g ulp)\n", k, (double)cs.means[(size_t)k], mean, off);
      ++bad;
    }
  }
  printf("means D=%d: %d of %d columns off; worst %.3f ulp of the column's largest |value|; least |mean| %.3g\n", D, bad, D,
         worst_ulps, least_abs_mean);
  if (!(least_abs_mean > 1.0)) {
    printf("means: the case is void, a column mean lies near 0\n");
    return 1;
  }
  return bad ? 1 : 0;
}

static int chunks_case(int D) {
  Case cs;
  cs.n = 150;   // two blocks, the second partial
  make_rows(cs.n, D, 1.0, &cs.x);
  if (int rc = run_device(D, true, &cs)) return rc;
  if ((int)cs.NM != nm_for(D)) return 1;
  size_t differ = 0;
  for (uint32_t i = 0; i < cs.np; ++i)
    for (uint32_t j = 0; j < cs.np; ++j) {   // (pad rows too: +inf norms and zero fragments, in both)
      uint32_t a, b;
      memcpy(&a, &cs.acc[(size_t)i * cs.np + j], 4);
      memcpy(&b, &cs.model[(size_t)i * cs.np + j], 4);
      differ += a != b;
    }
  printf("chunks D=%d NM=%u (NM mod %d = %u): %zu of %zu accumulators differ from the one-MFMA-at-a-time model\n", D, cs.NM, kWideKC,
         cs.NM % kWideKC, differ, (size_t)cs.np * cs.np);
  return differ ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "--band") == 0) {
    const int D = atoi(argv[2]);
    const float M = (float)atof(argv[3]);
    const Scale sc = make_scale(pick_scale_nn(M));
    const WideBand b = wide_band(M * sc.s2, D, sc);
    printf("band %d %.9g %.9g %.9g\n", D, (double)sc.s2, (double)b.e0, (double)b.kappa);
    return 0;
  }
  if (argc == 6 && strcmp(argv[1], "--units") == 0) {
    // "--units GQ GS RB QB": the unit map of a gq x gs group over RB reference blocks and QB query blocks, as
    // "shares S" / "grid G" and one line "id q_block share" per workgroup
    const WideGroup grp{(uint32_t)strtoul(argv[2], nullptr, 10), (uint32_t)strtoul(argv[3], nullptr, 10)};
    const uint32_t rb = (uint32_t)strtoul(argv[4], nullptr, 10), q_blocks = (uint32_t)strtoul(argv[5], nullptr, 10);
    const uint32_t n_shares = wide_shares(rb, grp), grid = wide_grid_size(q_blocks, n_shares, grp);
    printf("shares %u\ngrid %u\n", n_shares, grid);
    for (uint32_t id = 0; id < grid; ++id) {
      const WideUnit u = wide_unit(id, n_shares, grp);
      printf("%u %u %u\n", id, u.q_block, u.share);
    }
    return 0;
  }
  int bad = 0;
  double worst_all = 0.0;
  for (int D : {257, 512, 1024})
    for (double scale : {1e-3, 1.0, 1e3}) {
      double w = 0.0;
      const int rc = band_case(D, scale, &w);
      if (rc == 2) return 2;
      bad |= rc;
      if (w > worst_all) worst_all = w;
    }
  printf("worst ratio over all cases: %.4f\n", worst_all);
  {
    const int rc = means_case();
    if (rc == 2) return 2;
    bad |= rc;
  }
  for (int D : {257, 261, 267, 272}) {
    const int rc = chunks_case(D);
    if (rc == 2) return 2;
    bad |= rc;
  }
  printf(bad ? "FAILED\n" : "OK\n");
  return bad;
}
