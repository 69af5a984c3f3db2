// dc_forest_host.hpp -- the host part of a Boruvka forest on the radius graph: what dc_hip_session_radius_forest
// (dc_session.hip) and dc_hip_radius_forest_wide (dc_capi.hip) do between two min-edge sweeps.  Host only, no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dc {

// every round at least halves the number of components that still have a partner: 64 rounds cannot be needed
constexpr uint32_t kForestMaxRounds = 64;

struct ForestHost {
  std::vector<uint32_t> frame_of;   // frame of every rank
  std::vector<uint32_t> parent;     // union-find over frame ids, the smaller id is the root (= the component's id)
  std::vector<uint32_t> comp;       // component id of every frame: the input of the next sweep
  size_t found = 0;                 // pairs written to `edges` so far

  // false: rank is not a permutation of 0..n-1
  bool init(const uint32_t* rank, size_t n) {
    frame_of.assign(n, 0xFFFFFFFFu);
    for (size_t i = 0; i < n; ++i) {
      if (rank[i] >= n || frame_of[rank[i]] != 0xFFFFFFFFu) return false;
      frame_of[rank[i]] = (uint32_t)i;
    }
    parent.resize(n);
    comp.resize(n);
    for (size_t i = 0; i < n; ++i) parent[i] = comp[i] = (uint32_t)i;
    found = 0;
    return true;
  }

  uint32_t find(uint32_t x) {
    uint32_t root = x;
    while (parent[root] != root) root = parent[root];
    while (parent[x] != root) {
      const uint32_t next = parent[x];
      parent[x] = root;
      x = next;
    }
    return root;
  }

  // one round's d_best -> the pairs that join two components, appended to edges; returns how many (0: the forest is
  // complete) and brings comp up to date
  size_t join(const unsigned long long* best, uint32_t* edges) {
    const size_t n = parent.size();
    size_t joined = 0;
    for (size_t c = 0; c < n; ++c) {
      if (best[c] == ~0ull) continue;
      const uint32_t a = frame_of[(uint32_t)(best[c] >> 32)], b = frame_of[(uint32_t)best[c]];
      const uint32_t ra = find(a), rb = find(b);
      if (ra == rb) continue;   // the partner component chose the same pair
      parent[std::max(ra, rb)] = std::min(ra, rb);
      edges[2 * found] = a;
      edges[2 * found + 1] = b;
      ++found;
      ++joined;
    }
    if (joined != 0)
      for (size_t i = 0; i < n; ++i) comp[i] = find((uint32_t)i);
    return joined;
  }
};

}  // namespace dc
