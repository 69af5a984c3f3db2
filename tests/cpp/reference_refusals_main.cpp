// The CPU-reachable refusals of the resident reference handles through the C API, with no Python in the process: a driver
// for a build of the library's host code under sanitizers (which cannot be loaded into python without a preload).
//
//   python tests/test_capi_reference_refusals.py --drive <this program>
//
// feeds it the rows of that test's grid on standard input and compares what it prints with the recorded table.  A row is
//   open <entry point> <n_cols> <n_ref> <max_batch> <max_radius> <ref: 0 null, 1 given> <out: 0|1> <workspace: none|short|full>
//   call <name of tests/test_capi_reference_refusals.py no_handle_calls()> <others: 0 null, 1 given>
// and the answer is one line: the status, a blank, dc_hip_last_error().  Pointers are fake and never dereferenced.
// Built by hand (no test builds it), from clustering_amd/csrc after the library, with the HIP compiler CXX = hipcc:
//   $CXX -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -I../../include -I../lib/obj \
//        -Xarch_host -fsanitize=address,undefined -c dc_capi.hip dc_assign.hip           (the host code of the bodies)
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -I../../include -c ../../tests/cpp/reference_refusals_main.cpp
//   $CXX --offload-arch=gfx950 -fsanitize=address,undefined -o refusals reference_refusals_main.o dc_capi.o dc_assign.o \
//        <the other dc_*.o of ../lib/obj>
#include "dc_density.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

static void* const FAKE = (void*)64;
static const size_t BIG = (size_t)1 << 40;

static void* p(bool given) { return given ? FAKE : nullptr; }

static int open_row(std::istringstream& in) {
  std::string name, radius, ws;
  size_t n_cols, n_ref, max_batch;
  int ref, out;
  in >> name >> n_cols >> n_ref >> max_batch >> radius >> ref >> out >> ws;
  const bool narrow = name == "dc_hip_reference_open_dev";
  const size_t need = narrow ? dc_hip_reference_workspace_bytes(n_ref, n_cols, max_batch)
                             : dc_hip_reference_wide_workspace_bytes(n_ref, n_cols, max_batch);
  void* d_ws = ws == "none" ? nullptr : FAKE;
  const size_t ws_bytes = ws == "none" ? 0 : (ws == "short" ? (need ? need : 1) - 1 : BIG);
  dc_reference* hn = (dc_reference*)0x1234;
  dc_reference_wide* hw = (dc_reference_wide*)0x1234;
  const int rc = narrow ? dc_hip_reference_open_dev((const float*)p(ref), n_ref, n_cols, max_batch, radius == "nan" ? NAN : std::stof(radius),
                                                    d_ws, ws_bytes, nullptr, out ? &hn : nullptr)
                        : dc_hip_reference_wide_open_dev((const float*)p(ref), n_ref, n_cols, max_batch, d_ws, ws_bytes, nullptr,
                                                         out ? &hw : nullptr);
  if (out && rc != DC_OK && (narrow ? (void*)hn : (void*)hw) != nullptr) return 1000;   // *out is NULL on a refusal
  return rc;
}

static int call_row(std::istringstream& in) {
  std::string name, rest;
  int o;
  in >> name;
  std::getline(in, rest);   // " (reference, out) 1": the name's qualifier, if any, then others
  o = rest.back() == '1';
  const bool wide = name.find("_wide_") != std::string::npos;
  float radius = 0.5f;
  uint64_t a = 0, b = 0, c64 = 0;
  uint32_t c32 = 0, d = 0, e = 0;
  if (name.find("dc_hip_assign_open") == 0) {
    const bool no_ref = rest.find("reference") != std::string::npos, no_out = rest.find("out") != std::string::npos;
    dc_assign* h = (dc_assign*)0x1234;
    const int rc = wide ? dc_hip_assign_open_wide_dev((dc_reference_wide*)p(!no_ref), (const int32_t*)p(o), o ? 7 : 0, o ? 0.5f : NAN, p(o),
                                                      o ? BIG : 0, nullptr, no_out ? nullptr : &h)
                        : dc_hip_assign_open_dev((dc_reference*)p(!no_ref), (const int32_t*)p(o), o ? 7 : 0, o ? 0.5f : NAN, p(o), o ? BIG : 0,
                                                 nullptr, no_out ? nullptr : &h);
    return (!no_out && h != nullptr) ? 1000 : rc;
  }
  const std::string step = name.substr(strlen(wide ? "dc_hip_reference_wide_" : "dc_hip_reference_"));
  uint32_t* u = (uint32_t*)p(o);
  float* f = (float*)p(o);
  if (step == "set_free_energies_dev")
    return wide ? dc_hip_reference_wide_set_free_energies_dev(nullptr, f, nullptr) : dc_hip_reference_set_free_energies_dev(nullptr, f, nullptr);
  if (step == "stage_dev") return wide ? dc_hip_reference_wide_stage_dev(nullptr, f, 5, nullptr) : dc_hip_reference_stage_dev(nullptr, f, 5, nullptr);
  if (step == "populations_dev")
    return wide ? dc_hip_reference_wide_populations_dev(nullptr, o ? &radius : nullptr, 1, u, nullptr)
                : dc_hip_reference_populations_dev(nullptr, o ? &radius : nullptr, 1, u, nullptr);
  if (step == "nearest_dev")
    return wide ? dc_hip_reference_wide_nearest_dev(nullptr, f, u, f, u, f, nullptr) : dc_hip_reference_nearest_dev(nullptr, f, u, f, u, f, nullptr);
  if (step == "info_dev")
    return wide ? dc_hip_reference_wide_info_dev(nullptr, o ? &a : nullptr, o ? &b : nullptr, o ? &c64 : nullptr, o ? &d : nullptr,
                                                 o ? &e : nullptr, nullptr)
                : dc_hip_reference_info_dev(nullptr, o ? &a : nullptr, o ? &b : nullptr, o ? &c32 : nullptr, o ? &d : nullptr, o ? &e : nullptr,
                                            nullptr);
  if (step == "order_dev") return wide ? dc_hip_reference_wide_order_dev(nullptr, u, u, nullptr) : dc_hip_reference_order_dev(nullptr, 0, u, u, nullptr);
  return 1001;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    const int rc = what == "open" ? open_row(in) : (what == "call" ? call_row(in) : 1002);
    printf("%d %s\n", rc, rc ? dc_hip_last_error() : "");
  }
  return 0;
}
