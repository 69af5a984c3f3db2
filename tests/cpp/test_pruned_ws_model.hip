// test_pruned_ws_model.hip -- host model of every index the pruned self sweeps of 1 - 64 columns form in their workspace
// (tests/test_pruned_ws_model.py runs it on the CPU; no HIP runtime call is made, no device code runs).
//
// The library's own host code runs here, not a copy of it: this file includes the translation units dc_mfma.hip and
// dc_sort.hip with hipLaunchKernelGGL and hipMemsetAsync replaced by recorders (hipFuncSetAttribute and hipGetLastError
// by constants).  mfma_prepare,
// launch_pop_pruned[_segment], launch_radius_pairs, launch_radius_min_edge and launch_nn_pruned[_segment] are then called
// with made-up device addresses; every launch arrives at on_launch() with the grid, the dynamic LDS and the argument
// values the real launch would have had.  For every kernel a checker states, FROM THE KERNEL'S OWN INDEXING (named beside
// it), which bytes behind each pointer the kernel may touch.  The model then asserts
//   containment   every such range lies inside the buffer it points into: the workspace of mfma_workspace_bytes(n, D)
//                 bytes, or the caller's array (coords, pops, pairs, free energies ...) at its documented size;
//   padded orders group_rows <= kMaxGroupRows, T_r <= Tp, T_q <= Tp, positions fit kPopQueuePosBits where a queue form runs;
//   aliases       two ranges of one call that overlap under different names must be a pair of kAliases below (in either
//                 order), and whoever wrote the bytes of a read last must have written them under the read's own name;
//   shares/units  pick_chunks gives 1 .. 64 shares and the regrouped boxes (box_t / rho_t) hold them; seg_groups, seg_group,
//                 seg_unit and seg_owns are consistent and the segments partition the groups;
//   launch bounds the block of every launch within the kernel's __launch_bounds__; dynamic LDS at least what the kernel's
//                 carve-up indexes and at most the CU's 160 KB -- 80 KB for pop_pruned_kernel, whose source states that rule.
// The sweeps' entry points are the library's too: dc_mfma_step.hip is included once per MFMA count (host pass only), so
// pop_pruned_dispatch / nn_pruned_dispatch and launch_pop_cross run as they stand and their launches -- the sweep kernels
// with their grids, shares and dynamic LDS, box_by_share_kernel, the merge fill and unpack kernels, pop_cross_kernel,
// pops_by_frame*_kernel, the fills of the counts by position and of the ticket counters -- arrive at on_launch like the
// others.  sweep_resident_slots' occupancy query is answered with its own fallback (eight workgroups).  An unknown kernel
// name is a failure: nothing a launcher starts goes unchecked.  A 64-lane transcription of the pair sink (sink_model) shows
// reserved == stored, and is held to three seeded differences.
// The switch settings (DC_POP_SYM, DC_SHARE_FLOOR ...) come from the environment through the library's sweep_switches().
// Prints "ok <launches checked> <calls>" and returns 0, or the first violations and 1.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace model {
struct Arg;
void on_launch(const char* kernel, dim3 grid, dim3 block, size_t smem, std::vector<Arg>&& args);
void on_memset(const void* p, size_t bytes);
template <class... A>
void launch(const char* kernel, dim3 grid, dim3 block, size_t smem, const A&... a);
}  // namespace model

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, smem, stream, ...) \
  ::model::launch(#kernel, dim3(grid), dim3(block), (size_t)(smem), __VA_ARGS__)
#define hipMemsetAsync(p, v, bytes, s) (::model::on_memset((p), (size_t)(bytes)), hipSuccess)
#define hipFuncSetAttribute(...) hipSuccess
#define hipGetLastError() hipSuccess
// (sweep_resident_slots asks the device how many workgroups fit: the failed query's fallback, one per XCD label, serves)
#define hipOccupancyMaxActiveBlocksPerMultiprocessor(...) hipErrorUnknown
#define hipDeviceGetAttribute(...) hipErrorUnknown
#define hipGetDevice(p) ((*(p) = 0), hipSuccess)

#ifndef DC_STEP_MASK
#define DC_STEP_MASK 8191u
#endif
#include "../../clustering_amd/csrc/dc_mfma.hip"
#include "../../clustering_amd/csrc/dc_sort.hip"

using namespace dc;

// ---- recorded arguments --------------------------------------------------------------------------------------------
namespace model {
struct Arg {
  uint64_t v = 0;   // pointer address, integer value or float bits
  QSeg q{1, 0, 1};
  SortRemap remap{nullptr, nullptr, 0, nullptr};
  uintptr_t p() const { return (uintptr_t)v; }
  uint32_t u() const { return (uint32_t)v; }
};
template <class T>
Arg to_arg(T* p) { Arg a; a.v = (uint64_t)(uintptr_t)p; return a; }
inline Arg to_arg(std::nullptr_t) { return Arg{}; }
inline Arg to_arg(float f) { Arg a; uint32_t b; memcpy(&b, &f, 4); a.v = b; return a; }
inline Arg to_arg(double) { return Arg{}; }
inline Arg to_arg(const QSeg& q) { Arg a; a.q = q; return a; }
inline Arg to_arg(const SortRemap& r) { Arg a; a.remap = r; return a; }
inline Arg to_arg(const Rad2&) { return Arg{}; }
inline Arg to_arg(const CompView&) { return Arg{}; }
inline Arg to_arg(const SweepArgs&) { return Arg{}; }   // (the unpruned sweeps: never started here)
static PopKernArgs g_pop_args;   // the one struct argument of the per-wave kernels, as last launched
static NnKernArgs g_nn_args;
inline Arg to_arg(const PopKernArgs& x) { g_pop_args = x; return Arg{}; }
inline Arg to_arg(const NnKernArgs& x) { g_nn_args = x; return Arg{}; }
template <class T, class = typename std::enable_if<std::is_integral<T>::value || std::is_enum<T>::value>::type>
Arg to_arg(T x) { Arg a; a.v = (uint64_t)x; return a; }
template <class... A>
void launch(const char* kernel, dim3 grid, dim3 block, size_t smem, const A&... a) {
  on_launch(kernel, grid, block, smem, std::vector<Arg>{to_arg(a)...});
}
}  // namespace model
using model::Arg;
using model::g_pop_args;
using model::g_nn_args;

// ---- made-up device buffers ----------------------------------------------------------------------------------------
struct Buf {
  const char* name;
  uintptr_t base;
  size_t bytes;
};
enum { kWs, kCoords, kPops, kPairs, kCount, kFe, kNnIdx, kNnD2, kHdIdx, kHdD2, kCompIn, kRankIn, kBest, kBufs };
static Buf g_buf[kBufs];
static void* buf_ptr(int b) { return (void*)g_buf[b].base; }
static void set_buf(int b, const char* name, size_t bytes) {
  g_buf[b] = Buf{name, ((uintptr_t)(b + 1)) << 44, bytes};   // 16 TiB apart: no workspace reaches its neighbour
}

// ---- the call under test and its accesses --------------------------------------------------------------------------
struct Access {
  int launch;
  std::string name;
  int buf;
  size_t off, bytes;
  bool write;
};
struct Call {
  std::string what;
  uint32_t n = 0, D = 0;
  Layout L;
  size_t ws_bytes = 0;
  std::vector<Access> acc;
  std::vector<std::string> kernels;   // by launch number
  int launches = 0;
  // what one kernel leaves for the next (the device reads these from memory; the model keeps them)
  uint32_t stats_blocks = 0, key_blocks = 0, n_pos_order = 0, n_pos_order_ref = 0, open_items = 0, box_shares = 1;
  PopPlan pp{};   // the plans of the call (plan_pop / plan_nn with the launcher's own inputs)
  NnPlan np{};
};
static Call g;
static long g_launches = 0, g_calls = 0;
static int g_failures = 0;

static void fail(const std::string& msg) {
  if (++g_failures <= 25) printf("FAIL [%s n=%u D=%u] %s\n", g.what.c_str(), g.n, g.D, msg.c_str());
}
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      char b_[512];                               \
      snprintf(b_, sizeof b_, __VA_ARGS__);       \
      fail(std::string(#cond) + ": " + b_);       \
    }                                             \
  } while (0)

// name of the layout region an offset of the workspace starts in (names only: the extents below never come from here)
static const char* layout_name(size_t off, size_t* next = nullptr) {
  const Layout& L = g.L;
  struct { size_t off; const char* name; } r[] = {
      {0, "hdr"}, {L.off_comp, "comp"}, {L.off_img, "img"}, {L.off_img_b, "img_b"}, {L.off_norm, "norm"}, {L.off_img_s, "img_s"},
      {L.off_norm_s, "norm_s"}, {L.off_fe_s, "fe_s"}, {L.off_perm, "perm"}, {L.off_invpos, "invpos"}, {L.off_pq, "pq"},
      {L.off_keys_in, "keys_in"}, {L.off_keys_out, "keys_out"}, {L.off_vals_in, "vals_in"}, {L.off_img_p, "img_p"},
      {L.off_norm_p, "norm_p"}, {L.off_perm_p, "perm_p"}, {L.off_box_p, "box_p"}, {L.off_img_q, "img_q"},
      {L.off_norm_q, "norm_q"}, {L.off_perm_q, "perm_q"}, {L.off_box_q, "box_q"}, {L.off_ferange_p, "ferange_p"},
      {L.off_rhorange_p, "rhorange_p"}, {L.off_coords_p, "coords_p"}, {L.off_merge64, "merge64"}, {L.off_box_t, "box_t"},
      {L.off_rho_t, "rho_t"}, {L.off_tile_comp, "tile_comp"}, {L.off_tile_comp_q, "tile_comp_q"}, {L.fixed_end, "temp"}};
  const char* name = "hdr";
  if (next) *next = g.ws_bytes;
  for (auto& e : r) {
    if (e.off <= off) name = e.name;
    if (e.off > off && next && e.off < *next) *next = e.off;
  }
  return name;
}

static int g_cur_launch = 0;
static std::string g_cur_kernel;
// bytes [p, p + bytes) touched under `name` (nullptr: the layout region p starts in; "temp" needs an explicit name)
static void touch(uintptr_t p, size_t bytes, bool write, const char* name = nullptr) {
  if (p == 0 || bytes == 0) return;
  int b = -1;
  for (int k = 0; k < kBufs; ++k)
    if (g_buf[k].base && p >= g_buf[k].base && p < g_buf[k].base + ((uintptr_t)1 << 43)) b = k;
  if (b < 0) {
    fail(g_cur_kernel + ": a pointer into no buffer of the call");
    return;
  }
  const size_t off = p - g_buf[b].base;
  std::string nm = name ? name : (b == kWs ? layout_name(off) : g_buf[b].name);
  if (b == kWs && !name && nm == "temp") nm = "temp (unnamed)";
  if (off + bytes > g_buf[b].bytes) {
    char m[400];
    snprintf(m, sizeof m, "%s: %s [%zu, %zu) leaves %s of %zu bytes", g_cur_kernel.c_str(), nm.c_str(), off, off + bytes,
             g_buf[b].name, g_buf[b].bytes);
    fail(m);
  }
  if ((int)g.kernels.size() <= g_cur_launch) g.kernels.resize(g_cur_launch + 1);
  g.kernels[g_cur_launch] = g_cur_kernel;
  if (b == kWs && off < g.L.fixed_end && nm != "pops_shared_pos") {
    // a range never runs into the next field of the layout, live in this call or not (the one declared exception: the
    // counts by position of the symmetric shared-operand sweeps, which span norm_s .. vals_in)
    size_t next = 0;
    (void)layout_name(off, &next);
    if (off + bytes > next) {
      char m[400];
      snprintf(m, sizeof m, "%s: %s [%zu, %zu) runs into the next region of the layout at %zu", g_cur_kernel.c_str(), nm.c_str(), off,
               off + bytes, next);
      fail(m);
    }
  }
  g.acc.push_back(Access{g_cur_launch, nm, b, off, bytes, write});
}
static void rd(const Arg& a, size_t bytes, const char* name = nullptr) { touch(a.p(), bytes, false, name); }
static void wr(const Arg& a, size_t bytes, const char* name = nullptr) { touch(a.p(), bytes, true, name); }

// ---- the declared aliases: two names whose ranges may overlap within one call, and why that is safe ------------------
// The pair is what is checked (in either order); `first` / `second` say which use comes first in the text of `why`.  What
// makes an alias safe is checked access by access in end_call: whoever wrote the bytes of a read last wrote them under the
// read's own name (one stream: launch order is execution order).
struct Alias {
  const char *first, *second, *why;
};
static const Alias kAliases[] = {
    // the sort's temp region (behind fixed_end), free until the sort:
    {"stats table", "claim table", "mfma_prepare writes one or the other; a claim follows a finished statistics pass of an earlier call"},
    {"stats table", "cnt_tab", "stats_kernel, stats_reduce_kernel, then order_key_kernel"},
    {"claim table", "cnt_tab", "claim_pre_kernel, claim_guard_kernel, then order_key_kernel"},
    {"stats table", "sort.table", "... then the sort"},
    {"stats table", "sort.tmp", "... then the sort"},
    {"claim table", "sort.table", "... then the sort"},
    {"claim table", "sort.tmp", "... then the sort"},
    {"cnt_tab", "sort.table", "order_key_kernel, order_meta_kernel (its last reader), then sort_hist_kernel"},
    {"cnt_tab", "sort.tmp", "order_key_kernel, order_meta_kernel, then the first scatter pass"},
    {"sort.table", "cnt_tab", "the sort of the reference order is over when order_own_queries counts the query rows"},
    {"sort.tmp", "cnt_tab", "the same"},
    {"sort.table", "sort.tmp", "two sorts of one call lay the temp region out for their own n (all rows, then the rows of a range): the second starts after the last pass of the first"},
    {"sort.tmp", "sort.table", "the same"},
    // the sort's three buffers after the sort:
    {"keys_in", "minedge comp", "gather_u32_kernel writes after the sort of the order (launch_radius_min_edge)"},
    {"keys_out", "minedge rank", "the same"},
    {"minedge comp", "keys_in", "never in one call (own-order queries come with no sink); listed for the row-range order's sort"},
    {"keys_in", "open list", "nn_open_kernel lists the open queries after the last sort of the call"},
    // counts by position of the symmetric shared-operand sweeps over norm_s .. vals_in, after the orders are built:
    {"keys_in", "pops_shared_pos", "the fill of the counts follows the last sort"},
    {"keys_out", "pops_shared_pos", "the same"},
    {"vals_in", "pops_shared_pos", "the same"},
    {"fe_s", "pops_shared_pos", "population calls do not order by free energy"},
    {"invpos", "pops_shared_pos", "the same"},
    // later radii of one populations call (prep == false) and the query order of a row range run no further sort of the
    // reference order; the sort of the query order reuses the three buffers after the reference order is complete
};
static bool alias_allowed(const std::string& a, const std::string& b) {
  for (auto& e : kAliases)
    if (a == e.first && b == e.second) return true;
  return false;
}

static void end_call() {
  // overlap of differently named ranges of one buffer
  std::vector<Access>& A = g.acc;
  // (collapse to one record per (name, buf): the hull of its extents)
  struct Hull {
    std::string name;
    int buf;
    size_t lo, hi;
  };
  std::vector<Hull> H;
  for (auto& a : A) {
    Hull* h = nullptr;
    for (auto& e : H)
      if (e.buf == a.buf && e.name == a.name) h = &e;
    if (!h) {
      H.push_back(Hull{a.name, a.buf, a.off, a.off + a.bytes});
      continue;
    }
    h->lo = std::min(h->lo, a.off);
    h->hi = std::max(h->hi, a.off + a.bytes);
  }
  for (size_t i = 0; i < H.size(); ++i)
    for (size_t j = i + 1; j < H.size(); ++j) {
      if (H[i].buf != H[j].buf) continue;
      const Hull &a = H[i], &b = H[j];
      if (a.lo >= b.hi || b.lo >= a.hi) continue;
      char m[400];
      if (!alias_allowed(a.name, b.name) && !alias_allowed(b.name, a.name)) {
        snprintf(m, sizeof m, "%s [%zu, %zu) and %s [%zu, %zu) of %s overlap and are not a declared alias", a.name.c_str(), a.lo,
                 a.hi, b.name.c_str(), b.lo, b.hi, g_buf[a.buf].name);
        fail(m);
      }
    }
  // the launch order that makes an alias safe, access by access: whoever wrote the bytes of a read last, wrote them
  // under the read's own name (a region handed to another use is filled again before its first owner reads it)
  for (size_t i = 0; i < A.size(); ++i) {
    const Access& a = A[i];
    if (a.write) continue;
    for (size_t j = i; j-- > 0;) {
      const Access& b = A[j];
      if (!b.write || b.buf != a.buf || b.launch >= a.launch || a.off >= b.off + b.bytes || b.off >= a.off + a.bytes) continue;
      if (b.name != a.name) {
        char m[400];
        snprintf(m, sizeof m, "%s reads %s [%zu, %zu) after %s wrote %s [%zu, %zu) over it", g.kernels[a.launch].c_str(), a.name.c_str(),
                 a.off, a.off + a.bytes, g.kernels[b.launch].c_str(), b.name.c_str(), b.off, b.off + b.bytes);
        fail(m);
      }
      break;
    }
  }
  g_launches += g.launches;
  ++g_calls;
}

static void begin_call(const std::string& what, uint32_t n, uint32_t D, int n_rad, size_t capacity) {
  g = Call{};
  g.what = what;
  g.n = n;
  g.D = D;
  g.L = make_layout(n, D);
  g.ws_bytes = mfma_workspace_bytes(n, D);
  set_buf(kWs, "the workspace", g.ws_bytes);
  set_buf(kCoords, "coords", sizeof(float) * (size_t)n * D);
  set_buf(kPops, "pops", sizeof(uint32_t) * (size_t)n * (size_t)std::max(n_rad, 1));
  set_buf(kPairs, "pairs", sizeof(uint2) * capacity);
  set_buf(kCount, "count", 8);
  set_buf(kFe, "fe", sizeof(float) * (size_t)n);
  set_buf(kNnIdx, "nn_idx", 4 * (size_t)n);
  set_buf(kNnD2, "nn_d2", 4 * (size_t)n);
  set_buf(kHdIdx, "hd_idx", 4 * (size_t)n);
  set_buf(kHdD2, "hd_d2", 4 * (size_t)n);
  set_buf(kCompIn, "comp (by frame)", 4 * (size_t)n);
  set_buf(kRankIn, "rank (by frame)", 4 * (size_t)n);
  set_buf(kBest, "best", 8 * (size_t)n);
}

// ---- the kernels' own indexing ---------------------------------------------------------------------------------------
static bool is(const char* k, const char* name) { return strcmp(k, name) == 0; }
static uintptr_t ws_at(size_t off) { return g_buf[kWs].base + off; }

static bool on_sweep_launch(const char* k, const std::string& kn, dim3 grid, dim3 block, size_t smem, const std::vector<Arg>& a);

namespace model {
void on_memset(const void* p, size_t bytes) {
  g_cur_launch = g.launches++;
  g_cur_kernel = "fill";
  // (hipMemsetAsync(p, v, bytes): bytes [p, p + bytes))
  const uintptr_t a = (uintptr_t)p;
  const bool temp = a >= ws_at(g.L.fixed_end) && a < ws_at(g.ws_bytes);
  if (a == ws_at(g.L.off_norm_s))
    touch(a, bytes, true, "pops_shared_pos");   // (pop_pruned_dispatch's fill of the counts by position of the shared forms)
  else if (a == ws_at(0) && bytes > kHdrBytes) {   // (mfma_prepare: header and component region in ONE fill)
    touch(a, kHdrBytes, true);
    touch(a + kHdrBytes, bytes - kHdrBytes, true, "comp");
  } else
    touch(a, bytes, true, temp ? "temp (unnamed)" : nullptr);
}

void on_launch(const char* k, dim3 grid, dim3 block, size_t smem, std::vector<Arg>&& a) {
  g_cur_launch = g.launches++;
  g_cur_kernel = k;
  const uint32_t n = g.n, D = g.D;
  const size_t G = (size_t)grid.x * grid.y * grid.z;
  CHECK(G >= 1 && grid.y <= 65535u && grid.z <= 65535u && block.x * block.y * block.z <= 1024u, "%s: grid %u x %u, block %u", k,
        grid.x, grid.y, block.x);
  CHECK(smem <= 160u * 1024u, "%s: %zu bytes of dynamic LDS", k, smem);
  {  // the threads per block each kernel DECLARES (__launch_bounds__ in dc_prep.hpp, dc_mfma.hip, dc_sort.hip,
     // dc_mfma_kernels.hpp, dc_mfma_shared.hpp, dc_mfma_msym.hpp, dc_mfma_nn_shared.hpp); none declared: the default, 1024
    static const struct { const char* prefix; uint32_t threads; } kBounds[] = {
        {"stats_kernel", 256}, {"stats_reduce_kernel", 1024}, {"claim_pre_kernel", 256}, {"claim_guard_kernel", 1024},
        {"components_kernel", 1024}, {"order_key_kernel", 256}, {"order_meta_kernel", 1024}, {"order_rows2_kernel", 256},
        {"sort_hist_kernel", 256}, {"sort_scan_kernel", 256}, {"sort_scatter_kernel", 256}, {"pop_cross_kernel", 64},
        {"nn_cross_kernel", 64}, {"kernel", 256} /* pop_pruned_kernel */, {"(pop_shared_kernel", 256}, {"(pop_msym_kernel", 256},
        {"(nn_shared_kernel", 256}, {"(nn_pruned_kernel<S, TQV, true>", 512}, {"(nn_pruned_kernel<S, TQV>", 256}};
    uint32_t bound = 1024;
    for (auto& e : kBounds)
      if (strncmp(k, e.prefix, strlen(e.prefix)) == 0 && (strlen(e.prefix) > 6 || strcmp(k, e.prefix) == 0)) bound = e.threads;
    CHECK(block.x * block.y * block.z <= bound, "%s: a block of %u threads, the kernel declares %u", k, block.x, bound);
  }
  if (is(k, "stats_kernel")) {
    // (coords, n_rows, D, hdr, cookie, table): table[c * gridDim.x + blockIdx.x] for c < D, and the 64-bit slots
    // kMaxCols, kMaxCols + 1, kMaxCols + 2 of every block: kStatsRow x gridDim.x doubles
    rd(a[0], 4 * (size_t)n * D);
    wr(a[3], kHdrBytes);
    wr(a[5], sizeof(double) * kStatsRow * G, "stats table");
    CHECK(a[1].u() == n && a[2].u() == D && block.x == 256, "stats_kernel's shape");
    g.stats_blocks = (uint32_t)G;
  } else if (is(k, "stats_reduce_kernel")) {
    // (hdr, table, n_rows, D): nb = hdr[kHdrStatsBlocks] = gridDim.x of stats_kernel; table[col * nb + b], col <= kMaxCols + 2
    wr(a[0], kHdrBytes);
    rd(a[1], sizeof(double) * kStatsRow * (size_t)g.stats_blocks, "stats table");
  } else if (is(k, "claim_pre_kernel")) {
    // (coords, total, fe, n_rows, tab): tab[b], tab[B + b], tab[2 B + b], B = gridDim.x
    rd(a[0], 4 * (size_t)a[1].v);
    rd(a[2], 4 * (size_t)n);
    wr(a[4], 8 * 3 * G, "claim table");
    CHECK(a[1].v == (uint64_t)n * D, "claim_pre_kernel's total");
  } else if (is(k, "claim_guard_kernel")) {
    // (hdr, cookie, tab, B, pruned, have_fe, D, comp, n_rows, ..): tab[0 .. 3 B); comp: the component region
    wr(a[0], kHdrBytes);
    rd(a[2], 8 * 3 * (size_t)a[3].u(), "claim table");
    wr(a[7], 4 * kCompWords);
    CHECK(a[3].u() <= kClaimBlocks, "claim blocks");
  } else if (is(k, "fe_key_kernel")) {
    // (fe, n_rows, keys, vals, hdr): keys[i], vals[i], i < n_rows (both null: the range of the free energies only)
    rd(a[0], 4 * (size_t)a[1].u());
    wr(a[2], 4 * (size_t)a[1].u());
    wr(a[3], 4 * (size_t)a[1].u());
    wr(a[4], kHdrBytes);
  } else if (is(k, "fine_mark_kernel")) {
    // (coords, n_rows, D, hdr, r_max, comp): one byte of the bitmap at comp + kCompBitmap, fx, fy < kCoarseDim * kFineSub
    rd(a[0], 4 * (size_t)n * D);
    rd(a[3], kHdrBytes);
    wr(a[5], 4 * (kCompBitmap + kCompBitmapWords));
    CHECK(G * block.x >= n, "fine_mark_kernel covers the rows");
  } else if (is(k, "components_kernel")) {
    // (hdr, means, D, r_max, n_rows, frames_per_cell, fine_bits, comp, ..): the component region; LDS: the cell map
    // (dynamic) + occ, label, obox, root_cell, cbox (static): "81 KB of the CU's 160"
    rd(a[0], kHdrBytes);
    wr(a[7], 4 * kCompWords);
    const size_t lds = smem + sizeof(uint32_t) * 2 * kMaxOccupied + sizeof(float4) * kMaxOccupied + sizeof(uint32_t) * (kMaxComp + 4 * kMaxComp + 4);
    CHECK(smem == sizeof(uint16_t) * kCoarseDim * kCoarseDim && lds <= 160u * 1024u && G == 1, "components_kernel: %zu bytes of LDS", lds);
  } else if (is(k, "order_key_kernel")) {
    // (coords, D, hdr, comp, fine_bits, i_from, i_to, keys, vals, n_total, fe, fe_bits, counts, measure, perm, tile_comp,
    //  n_pos): grid-stride over max(i_to - i_from, n_pos) items: keys[j], vals[j] for j < i_to - i_from; perm[j] for j <
    //  n_pos; tile_comp[j] for j < n_pos / 32; counts[blockIdx.x * kMaxComp + c]: gridDim.x rows
    const uint32_t i_from = a[5].u(), i_to = a[6].u(), n_pos = a[16].u();
    rd(a[0], 4 * (size_t)i_to * D);
    wr(a[2], kHdrBytes);
    rd(a[3], 4 * kCompWords);
    wr(a[7], 4 * (size_t)(i_to - i_from));
    wr(a[8], 4 * (size_t)(i_to - i_from));
    rd(a[10], 4 * (size_t)a[9].u());
    wr(a[12], 4 * (size_t)kMaxComp * G, "cnt_tab");
    wr(a[14], 4 * (size_t)n_pos);
    wr(a[15], 4 * (size_t)(n_pos / 32));
    CHECK(i_to <= n && i_from <= i_to && a[9].u() == n && n_pos % 32 == 0 && n_pos <= 32u * g.L.Tp, "order_key_kernel: rows [%u, %u), %u positions", i_from, i_to, n_pos);
    CHECK(smem == order_key_smem(D, a[13].v != 0), "order_key_kernel's LDS");
    g.key_blocks = (uint32_t)G;
    g.n_pos_order = n_pos;
    if (a[14].p() == ws_at(g.L.off_perm_p)) g.n_pos_order_ref = n_pos;
  } else if (is(k, "order_meta_kernel")) {
    // (hdr, comp, table, n_blocks, start, range, base, n, group_rows, ..): table[b * kMaxComp + c], b < n_blocks; start and
    // base [kMaxComp + 1], range [kMaxComp + 1][2]; the padded order it lays out: sum of ceil(k_c / group_rows) group_rows
    // <= n + kMaxComp (group_rows - 1) positions
    wr(a[0], kHdrBytes);
    rd(a[2], 4 * (size_t)kMaxComp * a[3].u(), "cnt_tab");
    wr(a[4], 4 * (kMaxComp + 1));
    wr(a[5], 4 * 2 * (kMaxComp + 1));
    wr(a[6], 4 * (kMaxComp + 1));
    CHECK(a[3].u() == g.key_blocks, "order_meta_kernel adds up %u rows, order_key_kernel wrote %u", a[3].u(), g.key_blocks);
    const uint32_t rows = a[7].u(), group_rows = a[8].u();
    CHECK(group_rows >= 32 && group_rows <= (uint32_t)kMaxGroupRows && group_rows % 32 == 0, "group_rows %u", group_rows);
    CHECK((size_t)rows + (size_t)kMaxComp * (group_rows - 1) <= g.n_pos_order, "the padded order of %u rows in groups of %u needs more than the %u positions preset", rows, group_rows, g.n_pos_order);
    for (int q = 4; q <= 6; ++q)
      CHECK(a[q].p() >= ws_at(g.L.off_comp) && a[q].p() + 8 * (kMaxComp + 1) <= ws_at(g.L.off_img), "start / range / base lie in the component region");
  } else if (is(k, "sort_hist_kernel")) {
    // (keys, n, shift, mask, table, n_blocks): keys[i], i < n; table[digit * n_blocks + blockIdx.x]
    rd(a[0], 4 * (size_t)a[1].u(), a[0].p() >= ws_at(g.L.fixed_end) ? "sort.tmp" : nullptr);
    wr(a[4], 4 * (size_t)kSortBins * a[5].u(), "sort.table");
    CHECK(G == a[5].u() && (size_t)a[5].u() * kSortTile >= a[1].u(), "sort_hist_kernel's blocks");
  } else if (is(k, "sort_scan_kernel")) {
    // (table, n_blocks, totals): table rows in place, totals[digit]
    wr(a[0], 4 * (size_t)kSortBins * a[1].u(), "sort.table");
    wr(a[2], 4 * kSortBins, "sort.table");
    CHECK(a[2].p() == a[0].p() + 4 * (size_t)kSortBins * a[1].u() && G == kSortBins, "the totals follow the table");
  } else if (is(k, "sort_scatter_kernel<false>") || is(k, "sort_scatter_kernel<true>")) {
    // (keys_in, vals_in, keys_out, vals_out, n, shift, mask, table, totals, n_blocks, remap): reads [0, n) of the inputs;
    // <false> writes [0, n) of both outputs; <true> writes vals_out[seg_base[s] + ..] -- a position of the padded order
    // order_meta_kernel laid out -- and remap.tags[position / 32]
    const size_t nn = a[4].u();
    auto tmp = [&](const Arg& x) { return x.p() >= ws_at(g.L.fixed_end) ? "sort.tmp" : (const char*)nullptr; };
    rd(a[0], 4 * nn, tmp(a[0]));
    rd(a[1], 4 * nn, tmp(a[1]));
    rd(a[7], 4 * (size_t)kSortBins * a[9].u(), "sort.table");
    rd(a[8], 4 * kSortBins, "sort.table");
    if (is(k, "sort_scatter_kernel<false>")) {
      wr(a[2], 4 * nn, tmp(a[2]));
      wr(a[3], 4 * nn, tmp(a[3]));
    } else {
      wr(a[3], 4 * (size_t)g.n_pos_order);
      touch((uintptr_t)a[10].remap.tags, 4 * (size_t)(g.n_pos_order / 32), true);
      touch((uintptr_t)a[10].remap.seg_start, 4 * (kMaxComp + 1), false);
      touch((uintptr_t)a[10].remap.seg_base, 4 * (kMaxComp + 1), false);
      CHECK(a[10].remap.n_seg == (uint32_t)kMaxComp, "segments of the remap");
    }
  } else if (is(k, "order_rows2_kernel")) {
    // (coords, D, NM, perm, T, coords_o, boxes, fe, fe_s, invpos, ferange, rhorange, tile_comp, origins, hdr, img_a, a_form,
    //  norms_a, img_b, norms_b, grp_tq, grp, hash_slots, zero_pos, zero_planes): a block per 256 positions of n_pos = 32 T:
    //  perm[pos]; coords_o[pos * D + k]; boxes[t], ferange[t], rhorange[t], tile_comp[t] for t < T; fe_s[pos]; invpos[frame];
    //  img_a / img_b [tile * NM * 64 + m * 64 + lane] uint4; norms[tile * 32 + r]; zero_pos[z * n_pos + pos]; hash_slots[64]
    const uint32_t NM = a[2].u(), T = a[4].u();
    const size_t n_pos = 32 * (size_t)T;
    CHECK(a[1].u() == D && NM == g.L.NM && T <= g.L.Tp && G * 256 >= n_pos, "order_rows2_kernel: %u tiles, %zu blocks", T, G);
    CHECK(smem == order_rows_smem(D), "order_rows2_kernel's LDS: %zu", smem);
    rd(a[0], 4 * (size_t)n * D);
    rd(a[3], 4 * n_pos);
    wr(a[5], 4 * n_pos * D);
    wr(a[6], 16 * (size_t)T);
    rd(a[7], 4 * (size_t)n);
    wr(a[8], 4 * n_pos);
    wr(a[9], 4 * (size_t)n);
    wr(a[10], 8 * (size_t)T);
    wr(a[11], 8 * (size_t)T);
    rd(a[12], 4 * (size_t)T);
    rd(a[13], 4 * (size_t)kMaxComp * kMaxCols);
    wr(a[14], kHdrBytes);
    wr(a[15], 16 * 64 * (size_t)T * NM);
    wr(a[17], 4 * n_pos);
    wr(a[18], 16 * 64 * (size_t)T * NM);
    wr(a[19], 4 * n_pos);
    wr(a[22], 8 * 64);
    wr(a[23], 4 * n_pos * a[24].u());
  } else if (is(k, "gather_u32_kernel")) {
    // (by_frame, perm, n, by_pos): by_pos[p], perm[p] for p < n; by_frame[perm[p]]: a frame id < n_rows
    rd(a[0], 4 * (size_t)n);
    rd(a[1], 4 * (size_t)a[2].u());
    wr(a[3], 4 * (size_t)a[2].u(), a[3].p() == ws_at(g.L.off_keys_in) ? "minedge comp" : "minedge rank");
    CHECK(G * block.x >= a[2].u(), "gather_u32_kernel covers the positions");
  } else if (is(k, "edges_to_frames_kernel")) {
    // (edges, count, capacity, perm): edges[k] for k < min(*count, capacity); perm[e.x], perm[e.y]: positions of the order
    wr(a[0], 8 * (size_t)a[2].v);
    rd(a[1], 8);
    rd(a[3], 4 * (size_t)g.n_pos_order);
  } else if (is(k, "pairs_from_pops_kernel")) {
    rd(a[0], 4 * (size_t)a[1].u());
    wr(a[2], 8);
  } else if (is(k, "halve_kernel")) {
    wr(a[0], 8);
  } else if (is(k, "edges_flag_kernel")) {
    rd(a[0], kHdrBytes);
    wr(a[1], 8);
  } else if (is(k, "nn_open_kernel")) {
    // (coords, n_rows, D, fe, invpos_r, perm_q, n_items, comp, group_rows, q_seg, hdr, nn_d2, hd_d2, nn_idx, hd_idx, merge64,
    //  list, count): invpos_r[i] (i < n_rows, only without perm_q), perm_q[j] for j < n_items; list[< n_items];
    //  merge64[i], merge64[n_rows + i]
    const uint32_t items = a[6].u();
    rd(a[0], 4 * (size_t)n * D);
    rd(a[3], 4 * (size_t)n);
    if (a[5].p() == 0) rd(a[4], 4 * (size_t)n);
    rd(a[5], 4 * (size_t)items);
    rd(a[7], 4 * kCompWords);
    for (int q = 11; q <= 14; ++q) rd(a[q], 4 * (size_t)n);
    wr(a[15], 8 * 2 * (size_t)n);
    wr(a[16], 4 * (size_t)std::min<uint32_t>(items, n), "open list");
    wr(a[17], 4);
    CHECK(G * block.x >= items && a[1].u() == n, "nn_open_kernel covers the items");
    g.open_items = std::min<uint32_t>(items, n);
  } else if (is(k, "nn_cross_kernel")) {
    // (coords, n_rows, n_cols, fe, coords_r, perm_r, box_r, ferange_r, fe_c, comp, hdr, open_list, open_count, T, merge64):
    // tiles t < T of the component ranges: box_r[t], ferange_r[t], perm_r[32 t + r], coords_r[(32 t + r) D + k], fe_c[32 t + r]
    const size_t T = a[13].u();
    rd(a[4], 4 * 32 * T * D);
    rd(a[5], 4 * 32 * T);
    rd(a[6], 16 * T);
    rd(a[7], 8 * T);
    rd(a[8], 4 * 32 * T);
    rd(a[11], 4 * (size_t)g.open_items, "open list");
    wr(a[14], 8 * 2 * (size_t)n);
    CHECK(T <= g.L.Tp, "nn_cross_kernel's tiles");
  } else if (is(k, "nn_cross_write_kernel")) {
    rd(a[2], 4 * (size_t)g.open_items, "open list");
    rd(a[4], 8 * 2 * (size_t)n);
    for (int q = 6; q <= 9; ++q) wr(a[q], 4 * (size_t)n);
  } else {
    std::string kn = k;
    if (!kn.empty() && kn[0] == '(') kn = kn.substr(1);
    kn = kn.substr(0, kn.find_first_of("<)"));
    if (!on_sweep_launch(k, kn, grid, block, smem, a)) fail(std::string("a launch the model has no checker for: ") + k);
  }
}
}  // namespace model

// ---- the sweeps' entry points: dc_mfma_step.hip itself, once per MFMA count ------------------------------------------
// The library's pop_pruned_step_N / nn_pruned_step_N call the real pop_pruned_dispatch<N> / nn_pruned_dispatch<N>
// (dc_mfma_kernels.hpp) under the recorder macros: the shares, the grids, the dynamic LDS, the fills and every pointer are
// what the library forms.  Host pass only: in the device pass nothing refers to the sweep kernels, so none of their
// device code is generated (no kernel is ever started here).
#if !defined(__HIP_DEVICE_COMPILE__)
#define DC_STEP 1
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 2
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 3
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 4
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 5
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 6
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 7
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 8
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 9
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 10
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 11
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 12
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
#define DC_STEP 13
#include "../../clustering_amd/csrc/dc_mfma_step.hip"
#undef DC_STEP
namespace dc {
void pop_against_sweep(const AgainstArgs&, uint32_t, const Rad2&, uint32_t*, hipStream_t) { fail("a cross sweep was started"); }
void nn_against_sweep(const NnAgainstArgs&, uint32_t, uint32_t*, float*, uint32_t*, float*, hipStream_t) { fail("a cross sweep was started"); }
}  // namespace dc
#endif

// the kernels' carve-ups of their dynamic LDS, from the library's constants
template <int S>
static size_t shared_smem_of(int tq, int nr) { return (size_t)kRing * kTileUnits<S> * 16 + sizeof(uint32_t) * 4 * shared_wave_words(tq, nr); }
static size_t shared_smem(int nm, int tq, int nr) {
  switch (nm) {
#define X_(SV) case SV: return shared_smem_of<SV>(tq, nr);
    DC_FOR_EACH_S(X_)
#undef X_
  }
  return 0;
}
static size_t msym_smem_nm(int nm, int nr) {
  switch (nm) {
    case 3: return nr == 4 ? msym_smem<3, 4>() : msym_smem<3, 8>();
    case 4: return nr == 4 ? msym_smem<4, 4>() : msym_smem<4, 8>();
    case 5: return nr == 4 ? msym_smem<5, 4>() : msym_smem<5, 8>();
    case 6: return nr == 4 ? msym_smem<6, 4>() : msym_smem<6, 8>();
    case 7: return nr == 4 ? msym_smem<7, 4>() : msym_smem<7, 8>();
    case 8: return nr == 4 ? msym_smem<8, 4>() : msym_smem<8, 8>();
  }
  return 0;
}
constexpr size_t kOnePerCu = 160u * 1024u;   // the LDS of a gfx950 CU: what every launch must fit (no other kernel states a tighter rule)
constexpr size_t kTwoPerCu = 80u * 1024u;   // "below 80 KB of LDS -- two blocks per CU": the rule stated at kListCap for pop_pruned_kernel alone

static void check_seg(uint32_t n_groups, QSeg q) {
  // seg_groups / seg_group / seg_unit / seg_owns on the groups of one launch
  const uint32_t own = seg_groups(n_groups, q);
  uint32_t counted = 0;
  for (uint32_t gidx = 0; gidx < n_groups && n_groups <= 4096; ++gidx)
    if (seg_owns(gidx, q)) {
      ++counted;
      CHECK(seg_group(seg_unit(gidx, q), q) == gidx && seg_unit(gidx, q) < own, "seg_unit / seg_group on group %u of %u", gidx, n_groups);
    }
  if (n_groups <= 4096) CHECK(counted == own, "seg_groups says %u, seg_owns %u of %u groups", own, counted, n_groups);
  for (uint32_t u = 0; u < own && own <= 4096; ++u)
    CHECK(seg_owns(seg_group(u, q), q) && seg_group(u, q) < n_groups && seg_unit(seg_group(u, q), q) == u, "seg_group on unit %u", u);
}

// the units of a launch of the per-wave kernels (for_each_unit): static -- gridDim.x = the block units rounded up to 8,
// gridDim.y the shares; ticketed -- a one-dimensional grid of at most units workgroups, the shares in tk.n_chunks, the
// eight counters in the header.  -> shares
static uint32_t check_units(const char* k, dim3 grid, uint32_t n_blocks, const SweepTickets& tk, uint32_t hdr_word) {
  uint32_t shares;
  if (tk.ctr) {
    shares = tk.n_chunks;
    CHECK(grid.y == 1 && grid.x >= 1 && (unsigned long long)grid.x <= std::max<unsigned long long>(1, (unsigned long long)n_blocks * shares),
          "%s: %u persistent workgroups for %u x %u units", k, grid.x, n_blocks, shares);
    CHECK((uintptr_t)tk.ctr == ws_at(4 * (size_t)hdr_word), "%s: the ticket counters' header words", k);
    touch((uintptr_t)tk.ctr, 4 * kSweepQueues, true);
    // every (block unit, share) is drawn exactly once from the eight queues (dc_sweep_units.hpp; cheap sizes only)
    if ((unsigned long long)n_blocks * shares <= 2048) {
      std::vector<int> seen((size_t)n_blocks * shares, 0);
      for (uint32_t q = 0; q < kSweepQueues; ++q)
        for (uint32_t t = 0;; ++t) {
          const SweepUnit u = sweep_unit(n_blocks, shares, q, t);
          if (u.blk == kNoUnit) break;
          if (u.blk < n_blocks && u.share < shares) ++seen[(size_t)u.share * n_blocks + u.blk];
        }
      for (int v : seen) CHECK(v == 1, "%s: a unit of %u x %u is drawn %d times", k, n_blocks, shares, v);
    }
  } else {
    shares = grid.y;
    CHECK(grid.x == grid_x8(n_blocks), "%s: static grid %u for %u block units", k, grid.x, n_blocks);
  }
  CHECK(shares >= 1 && shares <= 64, "%s: %u shares", k, shares);
  return shares;
}

static const char* counts_name(uintptr_t p) {   // the counts by position of the symmetric sweeps
  return p == ws_at(g.L.off_pq) ? "pq" : p == ws_at(g.L.off_norm_s) ? "pops_shared_pos" : (const char*)nullptr;
}

// the launches inside pop_pruned_dispatch / nn_pruned_dispatch / launch_pop_cross; kn: the kernel's name without its
// template arguments ("kernel": the per-wave population kernel, which its launcher holds in a variable of that name)
static bool on_sweep_launch(const char* k, const std::string& kn, dim3 grid, dim3 block, size_t smem, const std::vector<Arg>& a) {
  const uint32_t n = g.n, D = g.D, NM = g.L.NM;
  const size_t G = (size_t)grid.x * grid.y * grid.z;
  auto ref_side = [&](uintptr_t img, uintptr_t norms, uintptr_t perm, uintptr_t box, uintptr_t rows, size_t T) {
    // tile t < T: img[(t NM + m) 64 + lane] uint4, norms[32 t + r], perm[32 t + r], box[t], rows[(32 t + r) D + k]
    touch(img, 16 * 64 * T * NM, false);
    touch(norms, 4 * 32 * T, false);
    touch(perm, 4 * 32 * T, false);
    touch(box, 16 * T, false);
    touch(rows, 4 * 32 * T * D, false);
  };
  auto query_side = [&](uintptr_t img, uintptr_t norms, uintptr_t perm, uintptr_t box, uintptr_t tile_comp, uint32_t n_q) {
    const size_t TQT = (n_q + 31) / 32;
    CHECK(n_q % 32 == 0 && TQT <= g.L.Tp, "%s: %u query positions, Tp %u", k, n_q, g.L.Tp);
    touch(img, 16 * 64 * TQT * NM, false);
    touch(norms, 4 * 32 * TQT, false);
    touch(perm, 4 * (size_t)n_q, false);
    touch(box, 16 * TQT, false);
    touch(tile_comp, 4 * TQT, false);
  };
  if (kn == "kernel") {   // pop_pruned_kernel<S, 1, TQ, MODE, SYM>(PopKernArgs)
    const PopKernArgs& A = g_pop_args;
    const PopPlan& pl = g.pp;
    const uint32_t wpb = block.x / 64, TQ = (uint32_t)tq_pop((int)NM), TQT = (A.n_q + 31) / 32;
    CHECK(block.x == 64 * pl.waves && block.x <= 256 && pl.tq == TQ && pl.group_tiles == TQ && pl.nr == 1 && A.n_rad == 1,
          "pop_pruned_kernel: block %u, plan of %u waves, %u tiles", block.x, pl.waves, pl.tq);
    CHECK(A.n_rows == n && A.n_cols == D && A.T <= g.L.Tp && A.CV.n_pos == 32u * A.T, "pop_pruned_kernel's shape");
    // pop_pruned_unit's carve-up of the dynamic LDS: per wave the survivor list [kListCap], the query rows [TQ * 32][n_cols],
    // the queues [TQ][kQueueCap][64]; and the rule stated at kListCap: below 80 KB, two workgroups per CU
    const size_t need = wpb * (sizeof(uint32_t) * kListCap + sizeof(float) * TQ * 32 * (size_t)D + sizeof(uint32_t) * TQ * kQueueCap * 64);
    CHECK(smem >= need && smem <= kTwoPerCu, "pop_pruned_kernel: %zu bytes of dynamic LDS, its carve-up needs %zu", smem, need);
    const uint32_t n_groups = (TQT + TQ - 1) / TQ;
    check_seg(n_groups, A.q_seg);
    (void)check_units(k, grid, (seg_groups(n_groups, A.q_seg) + wpb - 1) / wpb, A.tk, kHdrTicketsPop);
    if (32u * A.T > kPopQueueMaxRows) CHECK(pl.form == kPopWave || pl.form == kPopPairs, "positions beyond %u bits with form %d", kPopQueuePosBits, (int)pl.form);
    ref_side((uintptr_t)A.img_r, (uintptr_t)A.norms_r, (uintptr_t)A.perm_r, (uintptr_t)A.box_r, (uintptr_t)A.coords_r, A.T);
    query_side((uintptr_t)A.img_q, (uintptr_t)A.norms_q, (uintptr_t)A.perm_q, (uintptr_t)A.box_q, (uintptr_t)A.CV.tile_comp_q, A.n_q);
    touch((uintptr_t)A.CV.range_r, 4 * 2 * (kMaxComp + 1), false);
    touch((uintptr_t)A.coords, 4 * (size_t)n * D, false);
    touch((uintptr_t)A.hdr, kHdrBytes, true);
    if (A.pops_pos) {
      CHECK(pl.form == kPopWaveSym, "counts by position with form %d", (int)pl.form);
      touch((uintptr_t)A.pops_pos, 4 * 32 * (size_t)A.T, true, counts_name((uintptr_t)A.pops_pos));   // pops_pos[position]
    } else {
      touch((uintptr_t)A.pops, 4 * (size_t)n, true);   // pops[rr * n_rows + frame], rr < n_rad = 1
    }
    if (A.sink.best) {
      CHECK(pl.form == kPopMinEdge && (size_t)n + kOrderPadRows <= kPopQueueMaxRows, "a min-edge sink with form %d", (int)pl.form);
      touch((uintptr_t)A.sink.comp, 4 * 32 * (size_t)A.T, false, "minedge comp");   // sink.comp[pos], sink.rank[pos], pos < 32 T
      touch((uintptr_t)A.sink.rank, 4 * 32 * (size_t)A.T, false, "minedge rank");
      touch((uintptr_t)A.sink.best, 8 * (size_t)n, true);                           // sink.best[component id]: a frame id
    }
    if (A.sink.edges) {
      CHECK(pl.form == kPopPairs && A.perm_q == A.perm_r, "a pair sink with form %d", (int)pl.form);
      touch((uintptr_t)A.sink.edges, 8 * (size_t)A.sink.capacity, true);   // finish / emit_edge: edges[idx] only for idx < capacity
      touch((uintptr_t)A.sink.count, 8, true);
    }
    return true;
  }
  if (kn == "pop_shared_kernel" || kn == "pop_msym_kernel") {
    // (coords, n_rows, n_cols, img_p, norms_p, box_p, coords_p, T, img_q, norms_q, perm_q, box_q, n_q, q_seg, hdr, chain_counter,
    //  rad2, n_rad, [pops, q_in_ref_order,] CV [, pops_shared_pos]); a workgroup of four waves is one group of 4 TQ tiles
    const PopPlan& pl = g.pp;
    const bool msym = kn == "pop_msym_kernel";
    const uint32_t T = a[7].u(), n_q = a[12].u(), TQ = pl.tq, TQT = (n_q + 31) / 32;
    CHECK(block.x == 256 && pl.waves == 4 && pl.group_tiles == 4 * TQ && TQ == (uint32_t)tq_shared((int)NM, pl.nr) && T <= g.L.Tp,
          "%s: the shared forms' groups", k);
    CHECK(32u * T <= kPopQueueMaxRows && a[17].u() <= (uint32_t)pl.nr, "%s: positions beyond the queue's bits, or %u radii of %d", k, a[17].u(), pl.nr);
    const uint32_t n_groups = (TQT + 4 * TQ - 1) / (4 * TQ);
    check_seg(n_groups, a[13].q);
    CHECK(grid.x == grid_x8(seg_groups(n_groups, a[13].q)) && grid.y >= 1 && grid.y <= 64, "%s: grid %u x %u", k, grid.x, grid.y);
    // the kernels' carve-up: the operand ring, (msym: the accumulators,) then per wave queue + ids + exact-path counts
    const size_t need = msym ? msym_smem_nm((int)NM, pl.nr) : shared_smem((int)NM, (int)TQ, pl.nr);
    CHECK(need > 0 && smem >= need && smem <= kOnePerCu, "%s: %zu bytes of dynamic LDS, its carve-up needs %zu", k, smem, need);
    touch(a[3].p(), 16 * 64 * (size_t)T * NM, false);
    touch(a[4].p(), 4 * 32 * (size_t)T, false);
    touch(a[5].p(), 16 * (size_t)T, false);
    touch(a[6].p(), 4 * 32 * (size_t)T * D, false);
    touch(a[8].p(), 16 * 64 * (size_t)TQT * NM, false);
    touch(a[9].p(), 4 * 32 * (size_t)TQT, false);
    touch(a[10].p(), 4 * (size_t)n_q, false);
    touch(a[11].p(), 16 * (size_t)TQT, false);
    touch(a[14].p(), kHdrBytes, true);
    if (msym) {
      touch(a[19].p(), 4 * 32 * (size_t)T * pl.nr, true, "pops_shared_pos");   // [tile][NR][32]
    } else if (a.size() > 21) {
      touch(a[21].p(), 4 * 32 * (size_t)T, true, "pops_shared_pos");           // [32 T], one radius
    } else {
      touch(a[18].p(), 4 * (size_t)n * a[17].u(), true);                       // pops[rr * n_rows + frame]
    }
    return true;
  }
  if (kn == "pops_by_frame_ms_kernel") {
    // (pops_pos, perm, n_pos, n_rows, n_rad, hdr, pops): pops_pos[(pos / 32 * NR + rr) * 32 + pos % 32], perm[pos], pops[rr n_rows + frame]
    const size_t n_pos = a[2].u();
    touch(a[0].p(), 4 * n_pos * g.pp.nr, false, "pops_shared_pos");
    touch(a[1].p(), 4 * n_pos, false);
    touch(a[6].p(), 4 * (size_t)n * a[4].u(), true);
    CHECK(G * block.x >= n_pos && a[3].u() == n, "%s covers the positions", k);
    return true;
  }
  if (kn == "pops_by_frame_kernel") {
    // (pops_pos, perm, n_pos, hdr, pops): pops[perm[pos]] = pops_pos[pos], pos < n_pos
    const size_t n_pos = a[2].u();
    touch(a[0].p(), 4 * n_pos, false, counts_name(a[0].p()));
    touch(a[1].p(), 4 * n_pos, false);
    touch(a[4].p(), 4 * (size_t)n, true);
    CHECK(G * block.x >= n_pos, "%s covers the positions", k);
    return true;
  }
  if (kn == "pop_cross_kernel") {
    // (coords, n_cols, coords_r, perm_r, box_r, perm_q, box_q, tile_comp_q, comp, T_q, group_tiles, q_seg, q_in_ref_order, rad2,
    //  n_rad, r2max, hdr, out, stride, by_position): a wave per query group; cnt[rr * group_rows + k] in a static array of
    //  kMaxGroupRows * kMaxRadiiPerLaunch words; reference tiles of the adjacent components (< the tiles of the order);
    //  out[rr * stride + pq] (1), out[(pq / 32) * stride * 32 + rr * 32 + pq % 32] (2), out[rr * stride + frame] (0)
    const size_t T_q = a[9].u(), T_r = g.n_pos_order_ref / 32, stride = (size_t)a[18].v;
    const uint32_t group_tiles = a[10].u(), n_rad = a[14].u(), by = a[19].u();
    CHECK(block.x == 64 && 32u * group_tiles <= (uint32_t)kMaxGroupRows && n_rad >= 1 && n_rad <= (uint32_t)kMaxRadiiPerLaunch, "%s: groups of %u tiles, %u radii", k, group_tiles, n_rad);
    CHECK(G == seg_groups((uint32_t)((T_q + group_tiles - 1) / group_tiles), a[11].q), "%s: a workgroup per owned group", k);
    touch(a[2].p(), 4 * 32 * T_r * D, false);
    touch(a[3].p(), 4 * 32 * T_r, false);
    touch(a[4].p(), 16 * T_r, false);
    touch(a[5].p(), 4 * 32 * T_q, false);
    touch(a[6].p(), 16 * T_q, false);
    touch(a[7].p(), 4 * T_q, false);
    touch(a[8].p(), 4 * kCompWords, false);
    touch(a[0].p(), 4 * (size_t)n * D, false);
    const size_t words = by == 2 ? T_q * stride * 32 : (n_rad - 1) * stride + (by == 1 ? 32 * T_q : (size_t)n);
    touch(a[17].p(), 4 * words, true, counts_name(a[17].p()));
    return true;
  }
  if (kn == "nn_merge_fill_kernel") {   // (merge64, n_rows): merge64[i], i < 2 n_rows
    touch(a[0].p(), 8 * 2 * (size_t)a[1].u(), true);
    CHECK(G * block.x >= 2 * (size_t)a[1].u() && a[1].u() == n, "%s covers the words", k);
    return true;
  }
  if (kn == "box_by_share_kernel") {
    // (box_r, T, n_chunks, box_t, rho_r, rho_t, tickets): box_t[(t % n_chunks) * stride + t / n_chunks], stride = ceil(T / n_chunks):
    // n_chunks * stride boxes, which is also all a share's scan reads (box_t + chunk * stride, at most stride entries)
    const size_t T = a[1].u(), nc = a[2].u(), stride = nc ? (T + nc - 1) / nc : 0;
    CHECK(nc >= 1 && nc <= 64 && G * block.x >= T && T <= g.L.Tp, "%s: %zu tiles in %zu shares", k, T, nc);
    touch(a[0].p(), 16 * T, false);
    touch(a[3].p(), 16 * nc * stride, true);
    if (a[4].p()) {
      touch(a[4].p(), 8 * T, false);
      touch(a[5].p(), 8 * nc * stride, true);
    }
    touch(a[6].p(), 4 * kSweepQueues, true);
    g.box_shares = (uint32_t)nc;
    return true;
  }
  if (kn == "nn_shared_kernel") {
    // (coords, n_rows, n_cols, fe, img_r, norms_r, perm_r, box_r, box_t, ferange_r, fe_c, coords_c, invpos_r, T, img_q, norms_q,
    //  perm_q, box_q, n_q, q_seg, full_range, cell2, hdr, chain_counter, merge64, nn_idx, nn_d2, hd_idx, hd_d2, CV)
    const NnPlan& pl = g.np;
    const size_t T = a[13].u();
    const uint32_t n_q = a[18].u(), TQT = (n_q + 31) / 32, TQ = pl.tq;
    CHECK(block.x == 256 && pl.form == kNnShared && TQ == (uint32_t)tq_wave((int)NM) && pl.group_tiles == 4 * TQ && T <= g.L.Tp, "%s: the shared neighbour sweep's groups", k);
    const uint32_t n_groups = (TQT + 4 * TQ - 1) / (4 * TQ);
    check_seg(n_groups, a[19].q);
    CHECK(grid.x == grid_x8(seg_groups(n_groups, a[19].q)) && grid.y == g.box_shares, "%s: grid %u x %u, boxes regrouped for %u shares", k, grid.x, grid.y, g.box_shares);
    CHECK(smem <= kOnePerCu, "%s: %zu bytes of dynamic LDS", k, smem);
    ref_side(a[4].p(), a[5].p(), a[6].p(), a[7].p(), a[11].p(), T);
    touch(a[8].p(), 16 * (size_t)grid.y * ((T + grid.y - 1) / grid.y), false);
    touch(a[9].p(), 8 * T, false);
    touch(a[10].p(), 4 * 32 * T, false);
    touch(a[12].p(), 4 * (size_t)n, false);
    query_side(a[14].p(), a[15].p(), a[16].p(), a[17].p(), 0, n_q);
    touch(a[22].p(), kHdrBytes, true);
    if (grid.y > 1) touch(a[24].p(), 8 * 2 * (size_t)n, true);
    for (int q = 25; q <= 28; ++q) touch(a[q].p(), 4 * (size_t)n, true);
    return true;
  }
  if (kn == "nn_pruned_kernel") {   // nn_pruned_kernel<S, TQV[, COOP]>(NnKernArgs)
    const NnKernArgs& A = g_nn_args;
    const NnPlan& pl = g.np;
    const bool coop = strstr(k, "true") != nullptr;
    const uint32_t TQ = (uint32_t)tq_nn((int)NM), TQT = (A.n_q + 31) / 32, n_groups = (TQT + TQ - 1) / TQ;
    CHECK(pl.form == kNnWave && pl.tq == TQ && pl.group_tiles == TQ && A.n_rows == n && A.n_cols == D && A.T <= g.L.Tp && A.CV.n_pos == 32u * A.T, "nn_pruned_kernel's shape");
    check_seg(n_groups, A.q_seg);
    uint32_t shares;
    if (coop) {   // launch bound 512: the shares of a group are the kNnCoopWaves waves of a workgroup, on the static grid
      CHECK(block.x == 64 * kNnCoopWaves && block.x <= 512 && A.tk.ctr == nullptr && grid.x == grid_x8(seg_groups(n_groups, A.q_seg)), "nn_pruned_kernel<COOP>: grid %u, block %u", grid.x, block.x);
      shares = grid.y * kNnCoopWaves;
    } else {
      const uint32_t wpb = block.x / 64;
      CHECK(block.x == 64 * pl.waves && block.x <= 256, "nn_pruned_kernel: block %u", block.x);
      shares = check_units(k, grid, (seg_groups(n_groups, A.q_seg) + wpb - 1) / wpb, A.tk, kHdrTicketsNn);
    }
    CHECK(shares == g.box_shares && shares <= 64, "nn_pruned_kernel: %u shares, boxes regrouped for %u", shares, g.box_shares);
    // (this kernel states no two-per-CU rule: 82 944 bytes at 63 and 64 columns with four waves; the CU's 160 KB must hold)
    CHECK(smem <= kOnePerCu, "nn_pruned_kernel: %zu bytes of dynamic LDS", smem);
    const size_t T = A.T, stride = (T + shares - 1) / shares;
    ref_side((uintptr_t)A.img_r, (uintptr_t)A.norms_r, (uintptr_t)A.perm_r, (uintptr_t)A.box_r, (uintptr_t)A.coords_c, T);
    touch((uintptr_t)A.box_t, 16 * shares * stride, false);
    touch((uintptr_t)A.rho_r, 8 * T, false);
    touch((uintptr_t)A.rho_t, 8 * shares * stride, false);
    touch((uintptr_t)A.ferange_r, 8 * T, false);
    touch((uintptr_t)A.fe_c, 4 * 32 * T, false);
    touch((uintptr_t)A.invpos_r, 4 * (size_t)n, false);
    touch((uintptr_t)A.fe, 4 * (size_t)n, false);
    query_side((uintptr_t)A.img_q, (uintptr_t)A.norms_q, (uintptr_t)A.perm_q, (uintptr_t)A.box_q, (uintptr_t)A.CV.tile_comp_q, A.n_q);
    touch((uintptr_t)A.CV.range_r, 4 * 2 * (kMaxComp + 1), false);
    touch((uintptr_t)A.hdr, kHdrBytes, true);
    if (shares > 1) touch((uintptr_t)A.merge64, 8 * 2 * (size_t)n, true);
    touch((uintptr_t)A.nn_idx, 4 * (size_t)n, true);
    touch((uintptr_t)A.nn_d2, 4 * (size_t)n, true);
    touch((uintptr_t)A.hd_idx, 4 * (size_t)n, true);
    touch((uintptr_t)A.hd_d2, 4 * (size_t)n, true);
    return true;
  }
  if (kn == "nn_merge_unpack_rows_kernel") {   // (merge64, invpos, n_rows, tq, q_seg, nn_idx, nn_d2, hd_idx, hd_d2): by frame
    touch(a[0].p(), 8 * 2 * (size_t)n, false);
    touch(a[1].p(), 4 * (size_t)n, false);
    for (int q = 5; q <= 8; ++q) touch(a[q].p(), 4 * (size_t)n, true);
    CHECK(G * block.x >= n && a[2].u() == n, "%s covers the rows", k);
    return true;
  }
  if (kn == "nn_merge_unpack_kernel") {   // (merge64, perm_q, n_q, n_rows, tq, q_seg, nn_idx, ..): perm_q[p], p < n_q
    touch(a[0].p(), 8 * 2 * (size_t)n, false);
    touch(a[1].p(), 4 * (size_t)a[2].u(), false);
    for (int q = 6; q <= 9; ++q) touch(a[q].p(), 4 * (size_t)n, true);
    CHECK(G * block.x >= a[2].u() && a[3].u() == n, "%s covers the positions", k);
    return true;
  }
  return false;
}

// ---- the grid ----------------------------------------------------------------------------------------------------------
static void layout_checks(uint32_t n, uint32_t D) {
  // the layout itself: offsets ascend, are 256-byte aligned where a fill or an image starts, and the temp region behind
  // fixed_end is what the sort of the padded orders asks for
  const Layout L = make_layout(n, D);
  const size_t ws = mfma_workspace_bytes(n, D);
  CHECK(ws == L.fixed_end + sort_temp_bytes((size_t)n + kOrderPadRows), "mfma_workspace_bytes");
  CHECK(L.Tp == L.T + kPadTiles && 32u * (size_t)kPadTiles == kOrderPadRows, "Tp");
  CHECK(L.off_img % 256 == 0 && L.off_comp == kHdrBytes && L.off_img >= L.off_comp + 4 * kCompWords, "header and component region are one fill");
  const size_t offs[] = {L.off_comp, L.off_img, L.off_img_b, L.off_norm, L.off_img_s, L.off_norm_s, L.off_fe_s, L.off_perm, L.off_invpos,
                         L.off_pq, L.off_keys_in, L.off_keys_out, L.off_vals_in, L.off_img_p, L.off_norm_p, L.off_perm_p, L.off_box_p,
                         L.off_img_q, L.off_norm_q, L.off_perm_q, L.off_box_q, L.off_ferange_p, L.off_rhorange_p, L.off_coords_p,
                         L.off_merge64, L.off_box_t, L.off_rho_t, L.off_tile_comp, L.off_tile_comp_q, L.fixed_end};
  for (size_t k = 1; k < sizeof offs / sizeof offs[0]; ++k) CHECK(offs[k - 1] < offs[k] && offs[k] % 16 == 0, "layout offsets ascend (%zu)", k);
  // pruned_ws names the same regions
  const PrunedWs W = pruned_ws(buf_ptr(kWs), L, n);
  CHECK((uintptr_t)W.cnt_tab == ws_at(L.fixed_end) && (uintptr_t)W.sort.tmp == ws_at(L.fixed_end) &&
            W.sort.tmp_bytes == sort_temp_bytes((size_t)n + kOrderPadRows) && (uintptr_t)W.perm_p == ws_at(L.off_perm_p) &&
            (uintptr_t)W.base_q + 4 * (kMaxComp + 1) <= ws_at(L.off_comp + 4 * kCompHash),
        "pruned_ws");
}

static void plan_checks(uint32_t n, uint32_t D) {
  const SweepSwitches& sw = sweep_switches();
  const Layout L = make_layout(n, D);
  for (int n_rad = 1; n_rad <= kMaxRadiiPerLaunch; ++n_rad)
    for (int kind = kCallAll; kind <= kCallSegment; ++kind)
      for (int sink = kSinkNone; sink <= kSinkMinEdge; ++sink) {
        const PopPlan p = plan_pop(n, D, n_rad, (CallKind)kind, (SinkMode)sink, sw);
        CHECK(pop_form_built(p.form, nm_for((int)D)) && 32u * p.group_tiles <= (uint32_t)kMaxGroupRows && p.group_tiles >= 1 &&
                  (p.nr == 1 || p.nr == 4 || p.nr == 8),
              "plan_pop(%d radii, kind %d, sink %d): form %d, %u tiles per group", n_rad, kind, sink, (int)p.form, p.group_tiles);
        for (uint32_t i_from : {0u, n / 2}) {
          const QueryPlan Q = query_plan(QuerySel{i_from, n, 0, 0}, n, p.group_tiles);
          CHECK(Q.T_r <= L.Tp && Q.T_q <= L.Tp && Q.group_rows <= (uint32_t)kMaxGroupRows, "query_plan: T_r %u T_q %u Tp %u", Q.T_r, Q.T_q, L.Tp);
        }
      }
  const NnPlan q = plan_nn(n, D, sw);
  CHECK(nn_form_built(q.form, nm_for((int)D)) && 32u * q.group_tiles <= (uint32_t)kMaxGroupRows, "plan_nn: form %d, %u tiles per group", (int)q.form, q.group_tiles);
  // the segments of a sharded run partition the groups of the padded order
  for (uint32_t Gs : {1u, 2u, 3u, 5u, 8u})
    for (uint32_t gt : {std::min(q.group_tiles, 16u), 16u}) {
      const QueryPlan Q = query_plan(QuerySel{0, n, 0, Gs}, n, gt);
      const uint32_t n_groups = (Q.T_r + gt - 1) / gt;
      uint32_t sum = 0;
      for (uint32_t s = 0; s < Gs; ++s) sum += seg_groups(n_groups, QSeg{Gs, s, seg_block(Gs)});
      CHECK(sum == n_groups, "the %u segments own %u of %u groups", Gs, sum, n_groups);
      if (n_groups <= 4096) {
        std::vector<int> owners(n_groups, 0);
        for (uint32_t s = 0; s < Gs; ++s)
          for (uint32_t gi = 0; gi < n_groups; ++gi) owners[gi] += seg_owns(gi, QSeg{Gs, s, seg_block(Gs)}) ? 1 : 0;
        for (uint32_t gi = 0; gi < n_groups; ++gi) CHECK(owners[gi] == 1, "group %u has %d owners among %u segments", gi, owners[gi], Gs);
      }
      // the block of a sharded neighbour sweep holds the most groups a segment owns
      CHECK(nn_block_rows(n, D, Gs) >= (size_t)seg_groups((32u * nn_order_tiles(n, D) + nn_group_rows(n, D) - 1) / nn_group_rows(n, D), QSeg{Gs, 0, seg_block(Gs)}) * nn_group_rows(n, D), "nn_block_rows");
    }
}

static void run_calls(uint32_t n, uint32_t D) {
  char what[160];
  const Rad2 rad2{{0.25f, 0.5f, 1.0f, 2.0f, 0.125f, 4.0f, 3.0f, 0.75f}};
  struct Sel { uint32_t i_from, i_to, seg, G; };
  std::vector<Sel> sels = {{0, n, 0, 0}, {n / 2, n / 2, 0, 0}, {n / 3, n / 3 + 1, 0, 0}, {n / 2, n, 0, 0}, {0, 0, 0, 0}};
  for (uint32_t Gs : {1u, 2u, 3u, 5u, 8u})
    for (uint32_t s = 0; s < Gs; ++s) sels.push_back(Sel{0, n, s, Gs});
  float* coords = (float*)nullptr;
  for (const Sel& s : sels) {
    if (s.i_from > n || s.i_to > n) continue;
    for (int n_rad = 1; n_rad <= kMaxRadiiPerLaunch; ++n_rad)
      for (int stats_valid = 0; stats_valid <= ((n_rad == 1 || n_rad == kMaxRadiiPerLaunch) ? 1 : 0); ++stats_valid) {
        // (DC_FLAG_STATS_VALID changes the preparation, not the sweep: with one radius and with eight)
        // populations: dc_hip_populations_dev / _segment_dev -- mfma_prepare, then the pruned launcher
        snprintf(what, sizeof what, "populations rows [%u, %u) segment %u of %u, %d radii%s", s.i_from, s.i_to, s.seg, s.G, n_rad, stats_valid ? ", stats valid" : "");
        begin_call(what, n, D, n_rad, 0);
        g.pp = plan_pop(n, D, n_rad, call_kind(QuerySel{s.i_from, s.i_to, s.seg, s.G}, n), kSinkNone, sweep_switches());
        coords = (float*)buf_ptr(kCoords);
        (void)mfma_prepare(coords, n, D, buf_ptr(kWs), nullptr, stats_valid != 0, true, nullptr);
        if (s.G)
          launch_pop_pruned_segment(coords, n, D, s.seg, s.G, rad2, n_rad, (uint32_t*)buf_ptr(kPops), buf_ptr(kWs), nullptr, !stats_valid);
        else
          launch_pop_pruned(coords, n, D, s.i_from, s.i_to, rad2, n_rad, (uint32_t*)buf_ptr(kPops), buf_ptr(kWs), nullptr, !stats_valid);
        end_call();
      }
    for (int reuse = 0; reuse <= 1; ++reuse) {
      // neighbours: dc_hip_nearest_neighbors_dev / _segment_dev (reuse: DC_FLAG_STATS_VALID, the claim with free energies)
      snprintf(what, sizeof what, "neighbours rows [%u, %u) segment %u of %u%s", s.i_from, s.i_to, s.seg, s.G, reuse ? ", components reused" : "");
      begin_call(what, n, D, 1, 0);
      g.np = plan_nn(n, D, sweep_switches());
      coords = (float*)buf_ptr(kCoords);
      (void)mfma_prepare(coords, n, D, buf_ptr(kWs), nullptr, reuse != 0, true, reuse ? (const float*)buf_ptr(kFe) : nullptr);
      if (s.G)
        launch_nn_pruned_segment(coords, n, D, (const float*)buf_ptr(kFe), s.seg, s.G, (uint32_t*)buf_ptr(kNnIdx), (float*)buf_ptr(kNnD2),
                                 (uint32_t*)buf_ptr(kHdIdx), (float*)buf_ptr(kHdD2), buf_ptr(kWs), nullptr, reuse != 0);
      else
        launch_nn_pruned(coords, n, D, (const float*)buf_ptr(kFe), s.i_from, s.i_to, (uint32_t*)buf_ptr(kNnIdx), (float*)buf_ptr(kNnD2),
                         (uint32_t*)buf_ptr(kHdIdx), (float*)buf_ptr(kHdD2), buf_ptr(kWs), nullptr, reuse != 0);
      end_call();
    }
    if (s.i_from == 0 && s.i_to == n && n <= kMinEdgeMaxRows) {
      // one round of the forest: dc_hip_radius_min_edge[_segment]_dev
      snprintf(what, sizeof what, "min-edge round, segment %u of %u", s.seg, s.G);
      begin_call(what, n, D, 1, 0);
      g.pp = plan_pop(n, D, 1, call_kind(QuerySel{0, n, s.seg, s.G}, n), kSinkMinEdge, sweep_switches());
      coords = (float*)buf_ptr(kCoords);
      (void)mfma_prepare(coords, n, D, buf_ptr(kWs), nullptr, false, true, nullptr);
      launch_radius_min_edge(coords, n, D, 1.0f, (const uint32_t*)buf_ptr(kCompIn), (const uint32_t*)buf_ptr(kRankIn),
                             (unsigned long long*)buf_ptr(kBest), (uint32_t*)buf_ptr(kPops), buf_ptr(kWs), nullptr, s.seg, s.G);
      end_call();
    }
  }
  // the pair list: dc_hip_radius_pairs_dev with no buffer, a buffer of one pair, of many
  for (size_t capacity : {(size_t)0, (size_t)1, (size_t)156771, (size_t)313542}) {
    snprintf(what, sizeof what, "pair list, capacity %zu", capacity);
    begin_call(what, n, D, 1, capacity);
    g.pp = plan_pop(n, D, 1, kCallAll, capacity ? kSinkPairs : kSinkNone, sweep_switches());
    coords = (float*)buf_ptr(kCoords);
    (void)mfma_prepare(coords, n, D, buf_ptr(kWs), nullptr, false, true, nullptr);
    launch_radius_pairs(coords, n, D, 2.0000002f, (uint32_t*)buf_ptr(kPops), capacity ? (uint2*)buf_ptr(kPairs) : nullptr, capacity,
                        (unsigned long long*)buf_ptr(kCount), buf_ptr(kWs), nullptr);
    end_call();
  }
}

// ---- the pair sink of a 64-lane wave (dc_mfma_kernels.hpp: the kSinkPairs branch of finish, and emit_edge) ------------
// A transcription of the two places where slots of the pair list are RESERVED (one atomicAdd on sink.count per wave) and
// STORED (each lane its own), run on arbitrary inside masks, live masks, pad positions, active sets, counts and capacities
// (0 and count > capacity included): the slots stored must be exactly the reserved ones below the capacity, each once, and
// none at or beyond it.  variant 0: the code as it stands.  1 .. 3: seeded differences between reservation and store (the
// leader reserves one slot too few; the reserving lane adds the prefix of lane 62; a store without its capacity test) --
// the model has to report each of them, or it proves nothing.
//   finish     all 64 lanes are there.  Lane l = (h, c): query c of the tile (pad queries load dead_const and pad reference
//              rows an infinite norm: never inside), the 16 reference rows of its half h.  inside is cut to the rows at a
//              smaller position than the query; k = popcount(inside); inclusive prefix sum by shfl_up; lane 63 reserves
//              incl[63]; lane l stores at base + incl[l] - k[l] + 0, 1, .. where that is < capacity.
//   emit_edge  called inside pop_flush's divergent slot loop: only lanes with k < count are there.  m = ballot(have) over
//              them; the lowest lane of m reserves popcount(m), its base is read with readlane; lane l stores at base +
//              mbcnt(m) where that is < capacity.
static long sink_model(int variant) {
  long mismatches = 0;
  uint64_t rng = 0x9E3779B97F4A7C15ull + (uint64_t)variant;
  auto next = [&] { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  for (int trial = 0; trial < 20000; ++trial) {
    unsigned long long count = next() % 300;   // what other waves reserved before
    const unsigned long long cap = trial % 7 == 0 ? 0 : next() % 700;
    std::vector<int> stored(4096, 0);
    const unsigned long long before = count;
    unsigned long long reserved = 0;
    if (trial & 1) {
      const uint64_t live_q = trial % 5 == 0 ? (next() & next()) : ~0ull;          // bit c: query c of the tile is a frame
      const uint32_t live_r = trial % 3 == 0 ? (uint32_t)next() : 0xFFFFFFFFu;     // bit row: reference row is a frame
      const uint32_t t = (uint32_t)(next() % 8), qtile = (uint32_t)(next() % 8);   // reference tile, query tile
      uint32_t k[64], incl[64];
      for (int l = 0; l < 64; ++l) {
        const int h = l >> 5, c = l & 31;
        const uint32_t pos_q = qtile * 32u + (uint32_t)c;
        uint32_t inside = 0;
        const uint32_t raw = ((uint32_t)next() & (uint32_t)next()) | (trial % 11 == 0 ? 0xFFFFu : 0u);
        for (int r = 0; r < 16; ++r) {
          const uint32_t row = (uint32_t)(16 * h + r);   // (which 16 rows a half holds does not matter to the slots)
          const bool in = ((raw >> r) & 1u) && ((live_q >> c) & 1ull) && ((live_r >> row) & 1u) && (32u * t + row < pos_q);
          inside |= in ? (0x80000000u >> (2 * r)) : 0u;
        }
        k[l] = (uint32_t)__builtin_popcount(inside);
      }
      uint32_t run = 0;
      for (int l = 0; l < 64; ++l) incl[l] = (run += k[l]);
      if (run != 0) {   // ballot(k != 0) != 0
        const unsigned long long base = count, add = variant == 2 ? incl[62] : incl[63];
        count += add;
        reserved = add;
        for (int l = 0; l < 64; ++l) {
          unsigned long long idx = base + (incl[l] - k[l]);
          for (uint32_t e = 0; e < k[l]; ++e, ++idx)
            if ((idx < cap || variant == 3) && idx < stored.size()) ++stored[idx];
        }
      }
    } else {
      const uint64_t active = trial % 3 == 0 ? next() : (next() | next());
      const uint64_t have = next() & (trial % 4 == 0 ? ~0ull : next()) & active;
      const uint64_t m = have;   // the ballot sees the active lanes only
      if (m != 0) {
        const int leader = __builtin_ctzll(m);
        if (!((active >> leader) & 1)) ++mismatches;   // (the lane whose base readlane fetches took part in the atomic)
        const unsigned long long base = count, add = (unsigned long long)__builtin_popcountll(m) - (variant == 1 ? 1 : 0);
        count += add;
        reserved = add;
        for (int l = 0; l < 64; ++l)
          if ((have >> l) & 1) {
            const uint32_t rank = (uint32_t)__builtin_popcountll(m & ((l == 0) ? 0ull : (~0ull >> (64 - l))));
            if ((base + rank < cap || variant == 3) && base + rank < stored.size()) ++stored[base + rank];
          }
      }
    }
    bool bad = count != before + reserved;
    for (unsigned long long i = 0; i < stored.size() && !bad; ++i)
      bad = stored[i] != ((i >= before && i < before + reserved && i < cap) ? 1 : 0);
    mismatches += bad ? 1 : 0;
  }
  return mismatches;
}

int main() {
  g = Call{};
  g.what = "pair sink of one wave";
  {
    const long ok = sink_model(0);
    CHECK(ok == 0, "reserved and stored slots differ in %ld of 20000 trials", ok);
    for (int v = 1; v <= 3; ++v) CHECK(sink_model(v) > 0, "the wave model does not see seeded difference %d", v);
  }
  // (65 and 97: T_r = 1 mod 64 with groups of 512 rows -- where 64 shares of regrouped boxes need the most pad boxes)
  const uint32_t rows[] = {1, 2, 31, 32, 33, 37, 65, 97, 511, 512, 513, 1999, 2000, 2001, 2047, 2048, 2049, 3000, 32767, 32768, 32769, 100000, 1000000,
                           (uint32_t)kMinEdgeMaxRows};
  std::vector<uint32_t> cols;
  for (int nm = 1; nm <= kMaxMfma; ++nm) {   // both ends of every MFMA count's column range
    int lo = 0, hi = 0;
    for (int c = 1; c <= kMaxCols; ++c)
      if (nm_for(c) == nm) {
        if (!lo) lo = c;
        hi = c;
      }
    if (!lo) {
      printf("FAIL no column count with %d MFMAs\n", nm);
      return 1;
    }
    cols.push_back((uint32_t)lo);
    if (hi != lo) cols.push_back((uint32_t)hi);
  }
  for (uint32_t n : rows)
    for (uint32_t D : cols) {
      g = Call{};
      g.what = "layout and plans";
      g.n = n;
      g.D = D;
      g.L = make_layout(n, D);
      g.ws_bytes = mfma_workspace_bytes(n, D);
      set_buf(kWs, "the workspace", g.ws_bytes);
      layout_checks(n, D);
      plan_checks(n, D);
      run_calls(n, D);
      if (g_failures > 25) break;
    }
  if (g_failures) {
    printf("%d failures\n", g_failures);
    return 1;
  }
  printf("ok %ld %ld\n", g_launches, g_calls);
  return 0;
}
