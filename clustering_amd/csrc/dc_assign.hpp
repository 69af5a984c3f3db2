// dc_assign.hpp -- what the assigner (dc_assign.hip; dc_hip_assign_*, dc_hip_assigner_*) needs of the
// rest of the library: the facts of a resident reference handle, whose structs live with their entry points in
// dc_capi.hip, and the host's free-energy table.
#pragma once
#include "../../include/dc_density.h"

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dc {

// a resident reference as its assigner sees it
struct ReferenceFacts {
  size_t n_ref = 0, n_cols = 0, max_batch = 0;
  bool has_fe = false;      // set_free_energies has run
  float r2max = 0.0f;       // the largest fl32(r * r) a population call takes (+inf: any)
};
ReferenceFacts reference_facts(const dc_reference* h);
ReferenceFacts reference_facts(const dc_reference_wide* h);

// table[p] = the free energy of population p on the scale of max_pop, for p = 0 .. table.size() - 1: the arithmetic of
// dc_hip_free_energies_dev / dc_hip_free_energies_scaled_dev (host libm, reciprocal hoisted)
void fe_table(std::vector<float>& table, uint32_t max_pop);

int set_error(int code, const char* msg);

}  // namespace dc
