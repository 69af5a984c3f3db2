// dc_assign.hpp -- what the assigner (dc_assign.hip; dc_hip_assign_*, dc_hip_assigner_*) needs of the
// rest of the library: the one struct behind both resident reference handles with the shared bodies of its steps
// (dc_capi.hip, "the resident reference handles"), and the host's free-energy table.
#pragma once
#include "../../include/dc_density.h"

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dc {

// what differs between the kinds of handle: a constant table of function pointers and names (dc_capi.hip)
struct ReferenceKind;
extern const ReferenceKind kReferenceNarrow, kReferenceWide;   // rows of 1..64 columns (4.29), of 65..256 (4.28)
extern const ReferenceKind kReferenceXWide;                    // ... of 257..1024 (4.36)

// a resident reference of any kind
struct ReferenceHandle {
  const ReferenceKind* kind = nullptr;
  const float* d_ref = nullptr;     // borrowed until close
  size_t n_ref = 0, n_cols = 0, max_batch = 0;
  float r2max = 0.0f;               // the largest fl32(r * r) a population call takes: fl32(max_radius^2), the population
                                    // scale was chosen for it (narrow); +inf, any (wide)
  void* d_ws = nullptr;             // borrowed until close
  const float* d_query = nullptr;   // borrowed from stage to the batch's last sweep
  size_t n_query = 0;
  bool staged = false, has_fe = false;   // has_fe: set_free_energies has run
  uint32_t preparations = 0;        // runs of the reference's half of the preparation
};

// The bodies of the handles' entry points, one per step for every kind: dc_hip_reference[_wide|_xwide]_<step>_dev is
// handle_<step>(its kind, ...).  k names the entry point in every refusal, a null handle's among them.
int handle_open(const ReferenceKind& k, const float* d_ref, size_t n_ref, size_t n_cols, size_t max_batch, float max_radius,
                void* d_ws, size_t ws_bytes, void* stream, ReferenceHandle** out);
int handle_set_free_energies(const ReferenceKind& k, ReferenceHandle* h, const float* d_fe_ref, void* stream);
int handle_stage(const ReferenceKind& k, ReferenceHandle* h, const float* d_query, size_t n_query, void* stream);
int handle_populations(const ReferenceKind& k, ReferenceHandle* h, const float* radii, size_t n_radii, uint32_t* d_pops,
                       void* stream);
int handle_nearest(const ReferenceKind& k, ReferenceHandle* h, const float* d_fe_query, uint32_t* d_nn_idx, float* d_nn_d2,
                   uint32_t* d_hd_idx, float* d_hd_d2, void* stream);

// table[p] = the free energy of population p on the scale of max_pop, for p = 0 .. table.size() - 1: the arithmetic of
// dc_hip_free_energies_dev / dc_hip_free_energies_scaled_dev (host libm, reciprocal hoisted)
void fe_table(std::vector<float>& table, uint32_t max_pop);

int set_error(int code, const char* msg);

// The public types of the three kinds (include/dc_density.h) stay distinct names and are never defined: a pointer to
// any is a ReferenceHandle* under that name.
inline ReferenceHandle* handle(dc_reference* h) { return reinterpret_cast<ReferenceHandle*>(h); }
inline ReferenceHandle* handle(dc_reference_wide* h) { return reinterpret_cast<ReferenceHandle*>(h); }
inline ReferenceHandle* handle(dc_reference_xwide* h) { return reinterpret_cast<ReferenceHandle*>(h); }

}  // namespace dc
