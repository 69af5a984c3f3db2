// dc_assign.hip -- assigning new frames to a clustered reference (include/dc_density.h "assigner").
//   dc_hip_assign_*    device level: one batch = stage, populations at the radius, free energies by table, nearest,
//                      state pick -- five stream-ordered steps on a resident reference handle of any kind (the one
//                      struct and the shared bodies of dc_assign.hpp), or on the per-call cross entry points
//   dc_hip_assigner_*  host level: owns the reference, its self sweep, the handle and two batch slots; uploads and
//                      downloads on a copy stream beside the sweeps
// Two kernels live here, both a row per lane; every sweep is the library's.
#include "dc_assign.hpp"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace {

int failf(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return dc::set_error(code, buf);
}

#define DC_ASSIGN_TRY(expr)                                                                                        \
  do {                                                                                                             \
    hipError_t _e = (expr);                                                                                        \
    if (_e != hipSuccess) return failf(DC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// fe[q] = table[min(pops[q], n_ref)]: the clamp keeps a corrupt count inside the table
__global__ void assign_fe_kernel(const uint32_t* __restrict__ pops, uint32_t n, const float* __restrict__ table, uint32_t n_ref,
                                 float* __restrict__ fe) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) fe[q] = table[min(pops[q], n_ref)];
}

// states[q] = states_ref[hd] if hd exists, else states_ref[nn], else 0 ("none" is n_ref + 1: any index past the
// reference counts as none, so nothing is read past states_ref)
__global__ void assign_pick_kernel(const uint32_t* __restrict__ nn_idx, const uint32_t* __restrict__ hd_idx,
                                   const int32_t* __restrict__ states_ref, uint32_t n, uint32_t n_ref, int32_t* __restrict__ states) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  uint32_t p = hd_idx[q];
  if (p >= n_ref) p = nn_idx[q];
  states[q] = p < n_ref ? states_ref[p] : 0;
}

constexpr uint32_t kThreads = 256;

// a reference no handle takes (rows wider than 1024 columns, rows of 257..1024 columns unless the open call asked for their
// resident reference, or a reference beyond the narrow handle's 2^24 positions): the per-call
// cross entry points under DC_VARIANT_AUTO behind the three steps a batch takes of a handle
struct CrossRef {
  const float* d_ref = nullptr;
  const float* d_fe_ref = nullptr;
  size_t n_ref = 0, n_cols = 0;
  void* d_ws = nullptr;
  size_t ws_bytes = 0;
  const float* d_query = nullptr;
  size_t n_query = 0;
};
int cross_stage(CrossRef* c, const float* d_query, size_t n_query) {
  c->d_query = d_query, c->n_query = n_query;
  return DC_OK;
}
int cross_populations(const CrossRef* c, const float* radii, size_t n_radii, uint32_t* d_pops, void* stream) {
  return dc_hip_populations_cross_dev(c->d_query, c->n_query, c->d_ref, c->n_ref, c->n_cols, radii, n_radii, 0, c->n_query, d_pops,
                                      c->d_ws, c->ws_bytes, DC_VARIANT_AUTO, stream);
}
int cross_nearest(const CrossRef* c, const float* d_fe_query, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2,
                  void* stream) {
  return dc_hip_nearest_neighbors_cross_dev(c->d_query, c->n_query, c->d_ref, c->n_ref, c->n_cols, d_fe_query, c->d_fe_ref, 0,
                                            c->n_query, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2, c->d_ws, c->ws_bytes, DC_VARIANT_AUTO,
                                            stream);
}

// the workspace: table [n_ref + 1] | states_ref [n_ref] | six per-batch arrays [max_batch], each part on a 256-byte boundary
constexpr size_t kAlign = 256;
size_t padded(size_t bytes) { return (bytes + kAlign - 1) / kAlign * kAlign; }
struct AssignLayout {
  size_t table, states, batch[6], total;
  AssignLayout(size_t n_ref, size_t max_batch) {
    table = 0;
    states = table + padded(sizeof(float) * (n_ref + 1));
    size_t at = states + padded(sizeof(int32_t) * n_ref);
    for (size_t& b : batch) b = at, at += padded(4 * max_batch);
    total = at;
  }
};

}  // namespace

struct dc_assign {
  dc::ReferenceHandle* ref = nullptr;   // borrowed: the handle of either kind that holds the reference, or
  CrossRef* cross = nullptr;            // ... where no handle takes it
  size_t n_ref = 0, max_batch = 0;
  float radius = 0.0f;
  float* h_table = nullptr;      // the table's host copy: pinned, alive until close (its upload is asynchronous)
  std::vector<float> table;      // ... and where no pinned memory was to be had
  const float* d_table = nullptr;
  const int32_t* d_states_ref = nullptr;
  uint32_t* d_scratch[6] = {};   // pops, fe, nn_idx, nn_d2, hd_idx, hd_d2 for the outputs a caller leaves NULL
};

namespace {

// f: a resident reference as its assigner sees it -- the counts, whether its free energies were set, the largest
// fl32(r * r) a population call takes: *ref, or a description of *cross
int assign_open(const char* fn, dc::ReferenceHandle* ref, CrossRef* cross, const dc::ReferenceHandle& f, const int32_t* d_states_ref,
                uint32_t max_pop, float radius, void* d_ws, size_t ws_bytes, void* stream, dc_assign** out) {
  if (!f.has_fe) return failf(DC_ERR_INVALID_ARGUMENT, "%s: the reference's free energies were never set", fn);
  if (max_pop == 0) return failf(DC_ERR_INVALID_ARGUMENT, "%s: max_pop must be positive", fn);
  if (!(radius >= 0.0f)) return failf(DC_ERR_INVALID_ARGUMENT, "%s: radius=%g must be a number >= 0", fn, (double)radius);
  if (radius * radius > f.r2max)
    return failf(DC_ERR_INVALID_ARGUMENT, "%s: radius=%g, the reference was opened for radii whose square is at most %g", fn,
                 (double)radius, (double)f.r2max);
  if (!d_states_ref) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer", fn);
  const size_t need = dc_hip_assign_workspace_bytes(f.n_ref, f.max_batch);
  if (!d_ws || ws_bytes < need) return failf(DC_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", fn, need, d_ws ? ws_bytes : 0);
  hipStream_t s = (hipStream_t)stream;
  const AssignLayout lay(f.n_ref, f.max_batch);
  dc_assign* a = new dc_assign;
  a->ref = ref, a->cross = cross, a->n_ref = f.n_ref, a->max_batch = f.max_batch, a->radius = radius;
  const size_t n_table = f.n_ref + 1;
  a->table.resize(n_table);
  dc::fe_table(a->table, max_pop);
  const float* src = a->table.data();
  if (hipHostMalloc((void**)&a->h_table, sizeof(float) * n_table, hipHostMallocDefault) == hipSuccess) {
    memcpy(a->h_table, a->table.data(), sizeof(float) * n_table);
    std::vector<float>().swap(a->table);
    src = a->h_table;
  } else {
    (void)hipGetLastError();
    a->h_table = nullptr;
  }
  char* base = (char*)d_ws;
  hipError_t e = hipMemcpyAsync(base + lay.table, src, sizeof(float) * n_table, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(base + lay.states, d_states_ref, sizeof(int32_t) * f.n_ref, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) {
    dc_hip_assign_close(a);
    return failf(DC_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  }
  a->d_table = (const float*)(base + lay.table);
  a->d_states_ref = (const int32_t*)(base + lay.states);
  for (int k = 0; k < 6; ++k) a->d_scratch[k] = (uint32_t*)(base + lay.batch[k]);
  *out = a;
  return DC_OK;
}

// dc_hip_assign_open[_wide|_xwide]_dev
int assign_open_on(const char* fn, dc::ReferenceHandle* ref, const int32_t* d_states_ref, uint32_t max_pop, float radius, void* d_ws,
                   size_t ws_bytes, void* stream, dc_assign** out) {
  if (!out) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer (out)", fn);
  *out = nullptr;
  if (!ref) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer (reference)", fn);
  return assign_open(fn, ref, nullptr, *ref, d_states_ref, max_pop, radius, d_ws, ws_bytes, stream, out);
}

}  // namespace

extern "C" {

size_t dc_hip_assign_workspace_bytes(size_t n_ref, size_t max_batch) {
  if (n_ref == 0 || max_batch == 0) return 0;
  return AssignLayout(n_ref, max_batch).total;
}

int dc_hip_assign_open_dev(dc_reference* ref, const int32_t* d_states_ref, uint32_t max_pop, float radius, void* d_ws,
                           size_t ws_bytes, void* stream, dc_assign** out) {
  return assign_open_on("dc_hip_assign_open_dev", dc::handle(ref), d_states_ref, max_pop, radius, d_ws, ws_bytes, stream, out);
}

int dc_hip_assign_open_wide_dev(dc_reference_wide* ref, const int32_t* d_states_ref, uint32_t max_pop, float radius, void* d_ws,
                                size_t ws_bytes, void* stream, dc_assign** out) {
  return assign_open_on("dc_hip_assign_open_wide_dev", dc::handle(ref), d_states_ref, max_pop, radius, d_ws, ws_bytes, stream, out);
}

int dc_hip_assign_open_xwide_dev(dc_reference_xwide* ref, const int32_t* d_states_ref, uint32_t max_pop, float radius, void* d_ws,
                                 size_t ws_bytes, void* stream, dc_assign** out) {
  return assign_open_on("dc_hip_assign_open_xwide_dev", dc::handle(ref), d_states_ref, max_pop, radius, d_ws, ws_bytes, stream, out);
}

void dc_hip_assign_close(dc_assign* a) {
  if (!a) return;
  if (a->h_table) (void)hipHostFree(a->h_table);
  delete a;
}

int dc_hip_assign_batch_dev(dc_assign* a, const float* d_query, size_t n_query, int32_t* d_states, uint32_t* d_pops, float* d_fe,
                            uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* stream) {
  const char* fn = "dc_hip_assign_batch_dev";
  if (!a) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer (assigner)", fn);
  if (n_query > a->max_batch)
    return failf(DC_ERR_INVALID_ARGUMENT, "%s: n_query=%zu, the reference was opened for batches of at most %zu", fn, n_query, a->max_batch);
  if (n_query == 0) return DC_OK;
  if (!d_query || !d_states) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer", fn);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* pops = d_pops ? d_pops : a->d_scratch[0];
  float* fe = d_fe ? d_fe : (float*)a->d_scratch[1];
  uint32_t* nn_idx = d_nn_idx ? d_nn_idx : a->d_scratch[2];
  float* nn_d2 = d_nn_d2 ? d_nn_d2 : (float*)a->d_scratch[3];
  uint32_t* hd_idx = d_hd_idx ? d_hd_idx : a->d_scratch[4];
  float* hd_d2 = d_hd_d2 ? d_hd_d2 : (float*)a->d_scratch[5];
  const uint32_t n = (uint32_t)n_query, n_ref = (uint32_t)a->n_ref, blocks = (n + kThreads - 1) / kThreads;
  dc::ReferenceHandle* r = a->ref;
  if (int rc = r ? dc::handle_stage(*r->kind, r, d_query, n_query, stream) : cross_stage(a->cross, d_query, n_query)) return rc;
  if (int rc = r ? dc::handle_populations(*r->kind, r, &a->radius, 1, pops, stream) : cross_populations(a->cross, &a->radius, 1, pops, stream))
    return rc;
  assign_fe_kernel<<<blocks, kThreads, 0, s>>>(pops, n, a->d_table, n_ref, fe);
  if (int rc = r ? dc::handle_nearest(*r->kind, r, fe, nn_idx, nn_d2, hd_idx, hd_d2, stream)
                 : cross_nearest(a->cross, fe, nn_idx, nn_d2, hd_idx, hd_d2, stream))
    return rc;
  assign_pick_kernel<<<blocks, kThreads, 0, s>>>(nn_idx, hd_idx, a->d_states_ref, n, n_ref, d_states);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return failf(DC_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  return DC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// host level: the reference, its handle and two batch slots behind host pointers
// ------------------------------------------------------------------------------------------
namespace {

struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) {
      (void)hipGetLastError();
      prev = -1;
    }
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// DC_ASSIGN_OVERLAP=0: copies and sweeps on one stream (a measurement switch; read once per process)
bool overlap_wanted() {
  static const bool on = [] {
    const char* v = getenv("DC_ASSIGN_OVERLAP");
    return !(v && v[0] == '0');
  }();
  return on;
}

constexpr int kOutputs = 7;   // states, pops, fe, nn_idx, nn_d2, hd_idx, hd_d2: 4 bytes a row each

struct Slot {
  float* h_query = nullptr;      // pinned [max_batch][n_cols]
  uint32_t* h_out = nullptr;     // pinned [kOutputs][rows of the chunk]
  float* d_query = nullptr;
  uint32_t* d_out = nullptr;
  hipEvent_t uploaded = nullptr, swept = nullptr, downloaded = nullptr;
  size_t lo = 0, n = 0;          // the chunk whose results h_out is to receive (n == 0: none)
};

}  // namespace

struct dc_assigner {
  int device = 0, path = 0;
  unsigned flags = 0;                              // DC_ASSIGNER_* of the open call
  size_t n_ref = 0, n_cols = 0, max_batch = 0;
  float radius = 0.0f;
  uint32_t max_pop = 0;
  hipStream_t compute = nullptr, copy = nullptr;   // (one stream under DC_ASSIGN_OVERLAP=0)
  std::vector<void*> bufs;                         // device memory, freed at close
  dc::ReferenceHandle* ref = nullptr;              // the handle of paths 0 (narrow), 1 (wide) and 3 (xwide)
  CrossRef cross;
  dc_assign* assign = nullptr;
  std::vector<uint32_t> pops_ref;
  std::vector<float> fe_ref;
  Slot slot[2];
};

namespace {

hipError_t dev_alloc(dc_assigner* a, void** p, size_t bytes) {
  *p = nullptr;
  hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 4));
  if (e == hipSuccess) a->bufs.push_back(*p);
  return e;
}

int assigner_build(dc_assigner* a, const char* fn, const float* ref, const int32_t* states_ref) {
  const size_t n_ref = a->n_ref, n_cols = a->n_cols, max_batch = a->max_batch;
  DC_ASSIGN_TRY(hipSetDevice(a->device));
  DC_ASSIGN_TRY(hipStreamCreate(&a->compute));
  if (overlap_wanted())
    DC_ASSIGN_TRY(hipStreamCreate(&a->copy));
  else
    a->copy = a->compute;
  hipStream_t s = a->compute;
  void *d_ref, *d_states, *d_pops, *d_fe;
  DC_ASSIGN_TRY(dev_alloc(a, &d_ref, sizeof(float) * n_ref * n_cols));
  DC_ASSIGN_TRY(dev_alloc(a, &d_states, sizeof(int32_t) * n_ref));
  DC_ASSIGN_TRY(dev_alloc(a, &d_pops, sizeof(uint32_t) * n_ref));
  DC_ASSIGN_TRY(dev_alloc(a, &d_fe, sizeof(float) * n_ref));
  DC_ASSIGN_TRY(hipMemcpyAsync(d_ref, ref, sizeof(float) * n_ref * n_cols, hipMemcpyHostToDevice, s));
  DC_ASSIGN_TRY(hipMemcpyAsync(d_states, states_ref, sizeof(int32_t) * n_ref, hipMemcpyHostToDevice, s));
  // the reference's self sweep at the radius, once: the pruned wide sweep at 65..256 columns, the pruned extra-wide one at
  // 257..1024 where the open call asked for the resident reference of those widths, "auto" otherwise
  const bool wide = n_cols >= 65 && n_cols <= 256;
  const bool xwide = (a->flags & DC_ASSIGNER_XWIDE_REFERENCE) != 0u && n_cols >= 257 && n_cols <= 1024;
  {
    const size_t ws = wide    ? dc_hip_wide_pruned_workspace_bytes(n_ref, n_cols, 1)
                      : xwide ? dc_hip_xwide_pruned_workspace_bytes(n_ref, n_cols, 1)
                              : dc_hip_workspace_bytes(n_ref, n_cols, 1);
    void* d_ws = nullptr;
    if (ws) DC_ASSIGN_TRY(hipMalloc(&d_ws, ws));
    int rc = wide    ? dc_hip_populations_wide_pruned_dev((const float*)d_ref, n_ref, n_cols, &a->radius, 1, 0, 0, (uint32_t*)d_pops, d_ws,
                                                          ws, s)
             : xwide ? dc_hip_populations_xwide_pruned_dev((const float*)d_ref, n_ref, n_cols, &a->radius, 1, 0, 0, (uint32_t*)d_pops,
                                                           d_ws, ws, s)
                     : dc_hip_populations_dev((const float*)d_ref, n_ref, n_cols, &a->radius, 1, 0, n_ref, (uint32_t*)d_pops, d_ws, ws,
                                              DC_VARIANT_AUTO, s);
    if (rc == DC_OK) rc = dc_hip_free_energies_dev((const uint32_t*)d_pops, n_ref, (float*)d_fe, &a->max_pop, s);   // (synchronises)
    if (d_ws) (void)hipFree(d_ws);
    if (rc) return rc;
  }
  a->pops_ref.resize(n_ref);
  a->fe_ref.resize(n_ref);
  DC_ASSIGN_TRY(hipMemcpyAsync(a->pops_ref.data(), d_pops, sizeof(uint32_t) * n_ref, hipMemcpyDeviceToHost, s));
  DC_ASSIGN_TRY(hipMemcpyAsync(a->fe_ref.data(), d_fe, sizeof(float) * n_ref, hipMemcpyDeviceToHost, s));
  DC_ASSIGN_TRY(hipStreamSynchronize(s));
  // the handle of the width, else the per-call entry points
  void *d_hws = nullptr, *d_aws = nullptr;
  const size_t aws = dc_hip_assign_workspace_bytes(n_ref, max_batch);
  DC_ASSIGN_TRY(dev_alloc(a, &d_aws, aws));
  a->path = wide ? 1 : (xwide ? 3 : (n_cols <= 64 ? 0 : 2));
  if (a->path != 2) {
    const bool narrow = a->path == 0;
    const dc::ReferenceKind& k = wide ? dc::kReferenceWide : (xwide ? dc::kReferenceXWide : dc::kReferenceNarrow);
    const size_t hws = (wide    ? dc_hip_reference_wide_workspace_bytes
                        : xwide ? dc_hip_reference_xwide_workspace_bytes
                                : dc_hip_reference_workspace_bytes)(n_ref, n_cols, max_batch);
    DC_ASSIGN_TRY(dev_alloc(a, &d_hws, hws));
    const int rc = dc::handle_open(k, (const float*)d_ref, n_ref, n_cols, max_batch, narrow ? a->radius : INFINITY, d_hws, hws, s, &a->ref);
    if (rc == DC_ERR_TOO_LARGE && narrow)
      a->path = 2;   // (a reference beyond the narrow handle's 2^24 positions: the per-call entry points serve it)
    else if (rc)
      return rc;
  }
  if (a->path != 2) {
    const char* open_fn = wide ? "dc_hip_assign_open_wide_dev" : (xwide ? "dc_hip_assign_open_xwide_dev" : "dc_hip_assign_open_dev");
    if (int rc = dc::handle_set_free_energies(*a->ref->kind, a->ref, (const float*)d_fe, s)) return rc;
    if (int rc = assign_open_on(open_fn, a->ref, (const int32_t*)d_states, a->max_pop, a->radius, d_aws, aws, s, &a->assign)) return rc;
  } else {
    CrossRef& c = a->cross;
    c.d_ref = (const float*)d_ref, c.d_fe_ref = (const float*)d_fe, c.n_ref = n_ref, c.n_cols = n_cols;
    c.ws_bytes = dc_hip_cross_workspace_bytes(max_batch, n_ref, n_cols);
    if (c.ws_bytes) DC_ASSIGN_TRY(dev_alloc(a, &c.d_ws, c.ws_bytes));
    dc::ReferenceHandle f;
    f.n_ref = n_ref, f.n_cols = n_cols, f.max_batch = max_batch, f.has_fe = true, f.r2max = INFINITY;
    if (int rc = assign_open(fn, nullptr, &c, f, (const int32_t*)d_states, a->max_pop, a->radius, d_aws, aws, s, &a->assign)) return rc;
  }
  for (Slot& sl : a->slot) {
    DC_ASSIGN_TRY(hipHostMalloc((void**)&sl.h_query, std::max<size_t>(sizeof(float) * max_batch * n_cols, 4), hipHostMallocDefault));
    DC_ASSIGN_TRY(hipHostMalloc((void**)&sl.h_out, 4 * kOutputs * max_batch, hipHostMallocDefault));
    DC_ASSIGN_TRY(dev_alloc(a, (void**)&sl.d_query, sizeof(float) * max_batch * n_cols));
    DC_ASSIGN_TRY(dev_alloc(a, (void**)&sl.d_out, 4 * kOutputs * max_batch));
    DC_ASSIGN_TRY(hipEventCreateWithFlags(&sl.uploaded, hipEventDisableTiming));
    DC_ASSIGN_TRY(hipEventCreateWithFlags(&sl.swept, hipEventDisableTiming));
    DC_ASSIGN_TRY(hipEventCreateWithFlags(&sl.downloaded, hipEventDisableTiming));
  }
  DC_ASSIGN_TRY(hipStreamSynchronize(s));
  return DC_OK;
}

// the results of the chunk a slot last downloaded, into the caller's arrays (waits for that download)
int slot_flush(Slot& sl, void* const* outs) {
  if (sl.n == 0) return DC_OK;
  DC_ASSIGN_TRY(hipEventSynchronize(sl.downloaded));
  for (int k = 0; k < kOutputs; ++k)
    if (outs[k]) memcpy((uint32_t*)outs[k] + sl.lo, sl.h_out + (size_t)k * sl.n, 4 * sl.n);
  sl.n = 0;
  return DC_OK;
}

int slot_upload(dc_assigner* a, Slot& sl, const float* queries, size_t lo, size_t n) {
  memcpy(sl.h_query, queries + lo * a->n_cols, sizeof(float) * n * a->n_cols);
  DC_ASSIGN_TRY(hipMemcpyAsync(sl.d_query, sl.h_query, sizeof(float) * n * a->n_cols, hipMemcpyHostToDevice, a->copy));
  DC_ASSIGN_TRY(hipEventRecord(sl.uploaded, a->copy));
  return DC_OK;
}

// The copy stream runs U0 U1 D0 U2 D1 ..., the compute stream S0 S1 S2 ...: D(k) waits for S(k), S(k) for U(k), so U(k + 1)
// and D(k - 1) run beside S(k).  A slot is taken again only after the host has seen its download.
int assign_chunks(dc_assigner* a, const float* queries, size_t n_query, void* const* outs) {
  const size_t mb = a->max_batch, n_chunks = (n_query + mb - 1) / mb;
  if (int rc = slot_upload(a, a->slot[0], queries, 0, std::min(mb, n_query))) return rc;
  for (size_t k = 0; k < n_chunks; ++k) {
    Slot& sl = a->slot[k & 1];
    const size_t lo = k * mb, n = std::min(mb, n_query - lo);
    DC_ASSIGN_TRY(hipStreamWaitEvent(a->compute, sl.uploaded, 0));
    uint32_t* o = sl.d_out;
    if (int rc = dc_hip_assign_batch_dev(a->assign, sl.d_query, n, (int32_t*)o, o + n, (float*)(o + 2 * n), o + 3 * n,
                                         (float*)(o + 4 * n), o + 5 * n, (float*)(o + 6 * n), a->compute))
      return rc;
    DC_ASSIGN_TRY(hipEventRecord(sl.swept, a->compute));
    if (k + 1 < n_chunks) {
      Slot& next = a->slot[(k + 1) & 1];
      if (int rc = slot_flush(next, outs)) return rc;   // (chunk k - 1, downloaded behind S(k - 1))
      if (int rc = slot_upload(a, next, queries, lo + mb, std::min(mb, n_query - lo - mb))) return rc;
    }
    DC_ASSIGN_TRY(hipStreamWaitEvent(a->copy, sl.swept, 0));
    DC_ASSIGN_TRY(hipMemcpyAsync(sl.h_out, sl.d_out, 4 * kOutputs * n, hipMemcpyDeviceToHost, a->copy));
    DC_ASSIGN_TRY(hipEventRecord(sl.downloaded, a->copy));
    sl.lo = lo, sl.n = n;
  }
  if (int rc = slot_flush(a->slot[n_chunks & 1], outs)) return rc;   // (the chunk before the last, if any)
  return slot_flush(a->slot[(n_chunks - 1) & 1], outs);
}

// dc_hip_assigner_open[_flags]
int assigner_open(const char* fn, const float* ref, size_t n_ref, size_t n_cols, const int32_t* states_ref, float radius,
                  size_t max_batch, int device, unsigned flags, dc_assigner** out) {
  if (!out) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer (out)", fn);
  *out = nullptr;
  if (flags & ~DC_ASSIGNER_XWIDE_REFERENCE) return failf(DC_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", fn, flags & ~DC_ASSIGNER_XWIDE_REFERENCE);
  if (n_cols == 0 || n_ref == 0 || max_batch == 0)
    return failf(DC_ERR_INVALID_ARGUMENT, "%s: n_ref=%zu, n_cols=%zu, max_batch=%zu must be positive", fn, n_ref, n_cols, max_batch);
  if (!ref || !states_ref) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer", fn);
  if (!(radius >= 0.0f)) return failf(DC_ERR_INVALID_ARGUMENT, "%s: radius=%g must be a number >= 0", fn, (double)radius);
  if (n_ref + 1 > (size_t)UINT32_MAX || max_batch > (size_t)UINT32_MAX)
    return failf(DC_ERR_TOO_LARGE, "%s: max_batch=%zu, n_ref=%zu: frame ids must fit uint32", fn, max_batch, n_ref);
  if (n_cols > (size_t)UINT32_MAX || max_batch * n_cols > (size_t)UINT32_MAX * 4ull || n_ref * n_cols > (size_t)UINT32_MAX * 4ull)
    return failf(DC_ERR_TOO_LARGE, "%s: n_rows*n_cols too large", fn);
  const int n_dev = dc_hip_device_count();
  if (n_dev < 0) return n_dev;
  if (n_dev == 0) return failf(DC_ERR_NO_DEVICE, "%s: no HIP device found", fn);
  if (device < 0 || device >= n_dev) return failf(DC_ERR_INVALID_ARGUMENT, "%s: device %d out of range [0,%d)", fn, device, n_dev);
  DeviceGuard guard;
  dc_assigner* a = new dc_assigner;
  a->device = device, a->n_ref = n_ref, a->n_cols = n_cols, a->max_batch = max_batch, a->radius = radius, a->flags = flags;
  if (int rc = assigner_build(a, fn, ref, states_ref)) {
    const std::string msg = dc_hip_last_error();   // (close may run calls of its own)
    dc_hip_assigner_close(a);
    return dc::set_error(rc, msg.c_str());
  }
  *out = a;
  return DC_OK;
}
}  // namespace

extern "C" {

// flags = 0 unless the environment holds DC_ASSIGN_XWIDE=1 (read at every open, as DC_SESSION_WIDE is for sessions)
int dc_hip_assigner_open(const float* ref, size_t n_ref, size_t n_cols, const int32_t* states_ref, float radius, size_t max_batch,
                         int device, dc_assigner** out) {
  const char* v = getenv("DC_ASSIGN_XWIDE");
  const unsigned flags = (v && v[0] == '1' && v[1] == '\0') ? DC_ASSIGNER_XWIDE_REFERENCE : 0u;
  return assigner_open("dc_hip_assigner_open", ref, n_ref, n_cols, states_ref, radius, max_batch, device, flags, out);
}

int dc_hip_assigner_open_flags(const float* ref, size_t n_ref, size_t n_cols, const int32_t* states_ref, float radius, size_t max_batch,
                               int device, unsigned flags, dc_assigner** out) {
  return assigner_open("dc_hip_assigner_open_flags", ref, n_ref, n_cols, states_ref, radius, max_batch, device, flags, out);
}

int dc_hip_assigner_reference(const dc_assigner* a, uint32_t* pops_ref, float* fe_ref, uint32_t* max_pop) {
  if (!a) return failf(DC_ERR_INVALID_ARGUMENT, "dc_hip_assigner_reference: null pointer (assigner)");
  if (pops_ref) memcpy(pops_ref, a->pops_ref.data(), sizeof(uint32_t) * a->n_ref);
  if (fe_ref) memcpy(fe_ref, a->fe_ref.data(), sizeof(float) * a->n_ref);
  if (max_pop) *max_pop = a->max_pop;
  return DC_OK;
}

int dc_hip_assigner_path(const dc_assigner* a) { return a ? a->path : -1; }

int dc_hip_assigner_assign(dc_assigner* a, const float* queries, size_t n_query, int32_t* states, uint32_t* pops, float* fe,
                           uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx, float* hd_d2) {
  const char* fn = "dc_hip_assigner_assign";
  if (!a) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer (assigner)", fn);
  if (n_query == 0) return DC_OK;
  if (!queries || !states) return failf(DC_ERR_INVALID_ARGUMENT, "%s: null pointer", fn);
  if (n_query > (size_t)UINT32_MAX * 4ull / a->n_cols) return failf(DC_ERR_TOO_LARGE, "%s: n_query*n_cols too large", fn);
  DeviceGuard guard;
  DC_ASSIGN_TRY(hipSetDevice(a->device));
  void* const outs[kOutputs] = {states, pops, fe, nn_idx, nn_d2, hd_idx, hd_d2};
  const int rc = assign_chunks(a, queries, n_query, outs);
  if (rc) {   // leave nothing in flight on the slots, and nothing of this call for the next one to flush
    (void)hipStreamSynchronize(a->compute);
    (void)hipStreamSynchronize(a->copy);
  }
  a->slot[0].n = a->slot[1].n = 0;
  return rc;
}

void dc_hip_assigner_close(dc_assigner* a) {
  if (!a) return;
  DeviceGuard guard;
  (void)hipSetDevice(a->device);
  if (a->compute) (void)hipStreamSynchronize(a->compute);
  if (a->copy) (void)hipStreamSynchronize(a->copy);
  dc_hip_assign_close(a->assign);
  delete a->ref;
  for (Slot& sl : a->slot) {
    if (sl.h_query) (void)hipHostFree(sl.h_query);
    if (sl.h_out) (void)hipHostFree(sl.h_out);
    if (sl.uploaded) (void)hipEventDestroy(sl.uploaded);
    if (sl.swept) (void)hipEventDestroy(sl.swept);
    if (sl.downloaded) (void)hipEventDestroy(sl.downloaded);
  }
  for (void* p : a->bufs) (void)hipFree(p);
  if (a->copy && a->copy != a->compute) (void)hipStreamDestroy(a->copy);
  if (a->compute) (void)hipStreamDestroy(a->compute);
  delete a;
}

}  // extern "C"
