// test_scale_host.hip -- host-side check of the population sweeps' scale rule (pick_scale_pop,
// dc_mfma_kernels.hpp): for data extents and radii over many orders of magnitude the chosen power of two is the
// LARGEST at which the guard band of the launch is <= 1 (what the two-bit epilogue assumes), the coordinates and
// the folded constant fit fp16 at that scale, and the split into two pieces reproduces a value to 2^-22 (or to
// 2^(-14-g) in absolute terms).  And the plans of the pruned sweeps (plan_pop / plan_nn) against a table of what the library
// chose before the planners existed, every plan within the forms that are built.  No device code runs: built with hipcc, run by tests/test_capi_symbols.py on CPU.
#include "../../clustering_amd/csrc/dc_mfma_kernels.hpp"

#include <stdio.h>
#include <string.h>

using namespace dc;

// The plan tables: shape, call kind, sink and switch -> form, radii per sweep, query tiles per group, waves per
// workgroup, shift steps.  C1 - C5 (C4 and C5: one segment of a sharded run), 1 - 13 MFMAs per chain at 1 / 2 / 3 / 5 / 8
// radii per launch (a call of nine radii launches eight and one), operand images just below and above 96 MiB at 5 MFMAs,
// 49 999 / 50 000 rows at 3 MFMAs with three radii, and the forcing switches inside the built forms.
struct PopRow {
  const char* sw;
  uint32_t n_rows, n_cols;
  int n_rad;
  CallKind kind;
  SinkMode sink;
  PopForm form;
  int nr;
  uint32_t group_tiles, waves;
  int shift_steps;
};
struct NnRow {
  const char* sw;
  uint32_t n_rows, n_cols;
  NnForm form;
  uint32_t group_tiles, waves;
};
const PopRow kPopRows[] = {
    {"", 10000, 5, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 100000, 10, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 1000000, 10, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 1000000, 10, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 5000000, 30, 8, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 4, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 4, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 2, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 4, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 4, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 5, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 5, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 4, 5, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 8, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 8, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 4, 8, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 4, 1, kCallAll, kSinkPairs, kPopPairs, 1, 6, 1, 0},
    {"", 200000, 4, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 6, 1, 0},
    {"", 200000, 4, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 6, 1, 0},
    {"", 200000, 10, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 10, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 2, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 10, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 10, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 5, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 5, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 10, 5, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 8, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 8, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"", 200000, 10, 8, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"", 200000, 10, 1, kCallAll, kSinkPairs, kPopPairs, 1, 6, 1, 0},
    {"", 200000, 10, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 6, 1, 0},
    {"", 200000, 10, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 6, 1, 0},
    {"", 200000, 15, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 15, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"", 200000, 15, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 15, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 15, 2, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"", 200000, 15, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 15, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 15, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 15, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 15, 5, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 15, 5, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 15, 5, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 15, 8, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 15, 8, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 15, 8, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 15, 1, kCallAll, kSinkPairs, kPopPairs, 1, 4, 4, 0},
    {"", 200000, 15, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 4, 4, 0},
    {"", 200000, 15, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 4, 4, 0},
    {"", 200000, 20, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 20, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"", 200000, 20, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 20, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 20, 2, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"", 200000, 20, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 20, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 20, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 20, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 20, 5, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 20, 5, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 20, 5, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 20, 8, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 20, 8, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 20, 8, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 20, 1, kCallAll, kSinkPairs, kPopPairs, 1, 4, 4, 0},
    {"", 200000, 20, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 4, 4, 0},
    {"", 200000, 20, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 4, 4, 0},
    {"", 200000, 26, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 26, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"", 200000, 26, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 200000, 26, 2, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 26, 2, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 26, 2, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 26, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 26, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 26, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 26, 5, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 26, 5, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 26, 5, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 26, 8, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 26, 8, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 26, 8, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 26, 1, kCallAll, kSinkPairs, kPopPairs, 1, 4, 4, 0},
    {"", 200000, 26, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 4, 4, 0},
    {"", 200000, 26, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 4, 4, 0},
    {"", 200000, 31, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 31, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 31, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 31, 2, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 31, 2, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 31, 2, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 31, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 31, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 31, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 31, 5, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 31, 5, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 31, 5, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 31, 8, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 31, 8, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 31, 8, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 31, 1, kCallAll, kSinkPairs, kPopPairs, 1, 2, 4, 0},
    {"", 200000, 31, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 31, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 36, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 36, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 36, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 36, 2, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 36, 2, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 36, 2, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 36, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 36, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 36, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 36, 5, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 36, 5, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 36, 5, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 36, 8, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 36, 8, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 36, 8, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 36, 1, kCallAll, kSinkPairs, kPopPairs, 1, 2, 4, 0},
    {"", 200000, 36, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 36, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 42, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 42, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 42, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 42, 2, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 42, 2, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 42, 2, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 42, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 42, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 200000, 42, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 200000, 42, 5, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 42, 5, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 42, 5, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 42, 8, kCallAll, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 42, 8, kCallRange, kSinkNone, kPopMulti, 8, 8, 4, 7},
    {"", 200000, 42, 8, kCallSegment, kSinkNone, kPopMsym, 8, 8, 4, 7},
    {"", 200000, 42, 1, kCallAll, kSinkPairs, kPopPairs, 1, 2, 4, 0},
    {"", 200000, 42, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 42, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 47, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 47, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 2, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 47, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 3, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 47, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 5, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 5, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 47, 5, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 8, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 8, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 47, 8, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 47, 1, kCallAll, kSinkPairs, kPopPairs, 1, 2, 4, 0},
    {"", 200000, 47, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 47, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 52, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 52, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 2, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 52, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 3, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 52, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 5, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 5, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 52, 5, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 8, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 8, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 52, 8, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 52, 1, kCallAll, kSinkPairs, kPopPairs, 1, 2, 4, 0},
    {"", 200000, 52, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 52, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 58, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 58, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 2, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 58, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 3, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 58, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 5, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 5, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 58, 5, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 8, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 8, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 58, 8, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 58, 1, kCallAll, kSinkPairs, kPopPairs, 1, 2, 4, 0},
    {"", 200000, 58, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 58, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 63, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 63, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 2, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 63, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 3, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 63, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 5, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 5, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 63, 5, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 8, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 8, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 63, 8, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 63, 1, kCallAll, kSinkPairs, kPopPairs, 1, 2, 4, 0},
    {"", 200000, 63, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 63, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 64, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 64, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 2, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 2, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 64, 2, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 3, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 64, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 5, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 5, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 64, 5, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 8, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 8, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"", 200000, 64, 8, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"", 200000, 64, 1, kCallAll, kSinkPairs, kPopPairs, 1, 2, 4, 0},
    {"", 200000, 64, 1, kCallAll, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 200000, 64, 1, kCallSegment, kSinkMinEdge, kPopMinEdge, 1, 2, 4, 0},
    {"", 629120, 26, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 629120, 26, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"", 629120, 26, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 629152, 26, 1, kCallAll, kSinkNone, kPopSharedSym, 1, 16, 4, 0},
    {"", 629152, 26, 1, kCallRange, kSinkNone, kPopShared, 1, 16, 4, 0},
    {"", 629152, 26, 1, kCallSegment, kSinkNone, kPopSharedSym, 1, 16, 4, 0},
    {"", 49999, 14, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 49999, 14, 3, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"", 49999, 14, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"", 50000, 14, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"", 50000, 14, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"", 50000, 14, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 14, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 14, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 14, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 26, 1, kCallAll, kSinkNone, kPopSharedSym, 1, 16, 4, 0},
    {"DC_POP_SHARED=1", 200000, 26, 1, kCallRange, kSinkNone, kPopShared, 1, 16, 4, 0},
    {"DC_POP_SHARED=1", 200000, 26, 1, kCallSegment, kSinkNone, kPopSharedSym, 1, 16, 4, 0},
    {"DC_POP_SHARED=1", 200000, 26, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 26, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 26, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 40, 1, kCallAll, kSinkNone, kPopSharedSym, 1, 8, 4, 0},
    {"DC_POP_SHARED=1", 200000, 40, 1, kCallRange, kSinkNone, kPopShared, 1, 8, 4, 0},
    {"DC_POP_SHARED=1", 200000, 40, 1, kCallSegment, kSinkNone, kPopSharedSym, 1, 8, 4, 0},
    {"DC_POP_SHARED=1", 200000, 40, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 40, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 200000, 40, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_POP_SHARED=1", 629152, 26, 1, kCallAll, kSinkNone, kPopSharedSym, 1, 16, 4, 0},
    {"DC_POP_SHARED=0", 200000, 4, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 4, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 4, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 4, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 4, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 4, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 10, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 10, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 10, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 10, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 10, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 10, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_POP_SHARED=0", 200000, 14, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 14, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 14, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 14, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 14, 3, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 14, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 26, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 26, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 26, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 26, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 26, 3, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 26, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_POP_SHARED=0", 200000, 40, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"DC_POP_SHARED=0", 200000, 40, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"DC_POP_SHARED=0", 200000, 40, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"DC_POP_SHARED=0", 200000, 40, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"DC_POP_SHARED=0", 200000, 40, 3, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"DC_POP_SHARED=0", 200000, 40, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"DC_POP_SHARED=0", 629152, 26, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=1", 200000, 4, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 4, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 4, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 4, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 4, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 4, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 10, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 10, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 10, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 10, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 10, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 10, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=1", 200000, 14, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=1", 200000, 14, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_NN_SHARED=1", 200000, 14, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=1", 200000, 14, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 200000, 14, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 200000, 14, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 200000, 26, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=1", 200000, 26, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_NN_SHARED=1", 200000, 26, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=1", 200000, 26, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 200000, 26, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 200000, 26, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 200000, 40, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"DC_NN_SHARED=1", 200000, 40, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"DC_NN_SHARED=1", 200000, 40, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"DC_NN_SHARED=1", 200000, 40, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 200000, 40, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 200000, 40, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=1", 629152, 26, 1, kCallAll, kSinkNone, kPopSharedSym, 1, 16, 4, 0},
    {"DC_NN_SHARED=0", 200000, 4, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 4, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 4, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 4, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 4, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 4, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 10, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 10, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 10, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 10, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 10, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 10, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 1, 0},
    {"DC_NN_SHARED=0", 200000, 14, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=0", 200000, 14, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_NN_SHARED=0", 200000, 14, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=0", 200000, 14, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 200000, 14, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 200000, 14, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 200000, 26, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=0", 200000, 26, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_NN_SHARED=0", 200000, 26, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 4, 0},
    {"DC_NN_SHARED=0", 200000, 26, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 200000, 26, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 200000, 26, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 200000, 40, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"DC_NN_SHARED=0", 200000, 40, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"DC_NN_SHARED=0", 200000, 40, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 4, 0},
    {"DC_NN_SHARED=0", 200000, 40, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 200000, 40, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 200000, 40, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_NN_SHARED=0", 629152, 26, 1, kCallAll, kSinkNone, kPopSharedSym, 1, 16, 4, 0},
    {"DC_POP_SYM=0", 200000, 4, 1, kCallAll, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 4, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 4, 1, kCallSegment, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 4, 3, kCallAll, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 4, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 4, 3, kCallSegment, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 10, 1, kCallAll, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 10, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 10, 1, kCallSegment, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 10, 3, kCallAll, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 10, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 10, 3, kCallSegment, kSinkNone, kPopWave, 1, 6, 1, 0},
    {"DC_POP_SYM=0", 200000, 14, 1, kCallAll, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SYM=0", 200000, 14, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SYM=0", 200000, 14, 1, kCallSegment, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SYM=0", 200000, 14, 3, kCallAll, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 200000, 14, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 200000, 14, 3, kCallSegment, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 200000, 26, 1, kCallAll, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SYM=0", 200000, 26, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SYM=0", 200000, 26, 1, kCallSegment, kSinkNone, kPopWave, 1, 4, 4, 0},
    {"DC_POP_SYM=0", 200000, 26, 3, kCallAll, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 200000, 26, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 200000, 26, 3, kCallSegment, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 200000, 40, 1, kCallAll, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"DC_POP_SYM=0", 200000, 40, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"DC_POP_SYM=0", 200000, 40, 1, kCallSegment, kSinkNone, kPopWave, 1, 2, 4, 0},
    {"DC_POP_SYM=0", 200000, 40, 3, kCallAll, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 200000, 40, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 200000, 40, 3, kCallSegment, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_POP_SYM=0", 629152, 26, 1, kCallAll, kSinkNone, kPopShared, 1, 16, 4, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 4, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 4, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 4, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 4, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 4, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 4, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 10, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 10, 1, kCallRange, kSinkNone, kPopWave, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 10, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 10, 3, kCallAll, kSinkNone, kPopWaveSym, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 10, 3, kCallRange, kSinkNone, kPopWave, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 10, 3, kCallSegment, kSinkNone, kPopWaveSym, 1, 6, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 14, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 14, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 14, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 14, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 200000, 14, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 200000, 14, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 200000, 26, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 4, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 26, 1, kCallRange, kSinkNone, kPopWave, 1, 4, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 26, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 4, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 26, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 200000, 26, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 200000, 26, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 200000, 40, 1, kCallAll, kSinkNone, kPopWaveSym, 1, 2, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 40, 1, kCallRange, kSinkNone, kPopWave, 1, 2, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 40, 1, kCallSegment, kSinkNone, kPopWaveSym, 1, 2, 2, 0},
    {"DC_WAVES_PER_GROUP=2", 200000, 40, 3, kCallAll, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 200000, 40, 3, kCallRange, kSinkNone, kPopMulti, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 200000, 40, 3, kCallSegment, kSinkNone, kPopMsym, 4, 8, 4, 3},
    {"DC_WAVES_PER_GROUP=2", 629152, 26, 1, kCallAll, kSinkNone, kPopSharedSym, 1, 16, 4, 0},
};
const NnRow kNnRows[] = {
    {"", 200000, 5, kNnWave, 6, 1},
    {"", 629120, 5, kNnWave, 6, 1},
    {"", 629152, 5, kNnWave, 6, 1},
    {"", 200000, 10, kNnWave, 6, 1},
    {"", 629120, 10, kNnWave, 6, 1},
    {"", 629152, 10, kNnWave, 6, 1},
    {"", 200000, 14, kNnWave, 4, 4},
    {"", 629120, 14, kNnWave, 4, 4},
    {"", 629152, 14, kNnWave, 4, 4},
    {"", 200000, 26, kNnWave, 4, 4},
    {"", 629120, 26, kNnWave, 4, 4},
    {"", 629152, 26, kNnShared, 16, 4},
    {"", 200000, 40, kNnWave, 2, 4},
    {"", 629120, 40, kNnShared, 8, 4},
    {"", 629152, 40, kNnShared, 8, 4},
    {"", 200000, 42, kNnWave, 2, 4},
    {"", 629120, 42, kNnShared, 8, 4},
    {"", 629152, 42, kNnShared, 8, 4},
    {"", 200000, 64, kNnWave, 2, 4},
    {"", 629120, 64, kNnWave, 2, 4},
    {"", 629152, 64, kNnWave, 2, 4},
    {"DC_NN_SHARED=1", 200000, 26, kNnShared, 16, 4},
    {"DC_NN_SHARED=1", 629120, 26, kNnShared, 16, 4},
    {"DC_NN_SHARED=1", 629152, 26, kNnShared, 16, 4},
    {"DC_NN_SHARED=1", 200000, 40, kNnShared, 8, 4},
    {"DC_NN_SHARED=1", 629120, 40, kNnShared, 8, 4},
    {"DC_NN_SHARED=1", 629152, 40, kNnShared, 8, 4},
    {"DC_NN_SHARED=1", 200000, 42, kNnShared, 8, 4},
    {"DC_NN_SHARED=1", 629120, 42, kNnShared, 8, 4},
    {"DC_NN_SHARED=1", 629152, 42, kNnShared, 8, 4},
    {"DC_NN_SHARED=1", 200000, 64, kNnWave, 2, 4},
    {"DC_NN_SHARED=1", 629120, 64, kNnWave, 2, 4},
    {"DC_NN_SHARED=1", 629152, 64, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 200000, 5, kNnWave, 6, 1},
    {"DC_NN_SHARED=0", 629120, 5, kNnWave, 6, 1},
    {"DC_NN_SHARED=0", 629152, 5, kNnWave, 6, 1},
    {"DC_NN_SHARED=0", 200000, 10, kNnWave, 6, 1},
    {"DC_NN_SHARED=0", 629120, 10, kNnWave, 6, 1},
    {"DC_NN_SHARED=0", 629152, 10, kNnWave, 6, 1},
    {"DC_NN_SHARED=0", 200000, 14, kNnWave, 4, 4},
    {"DC_NN_SHARED=0", 629120, 14, kNnWave, 4, 4},
    {"DC_NN_SHARED=0", 629152, 14, kNnWave, 4, 4},
    {"DC_NN_SHARED=0", 200000, 26, kNnWave, 4, 4},
    {"DC_NN_SHARED=0", 629120, 26, kNnWave, 4, 4},
    {"DC_NN_SHARED=0", 629152, 26, kNnWave, 4, 4},
    {"DC_NN_SHARED=0", 200000, 40, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 629120, 40, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 629152, 40, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 200000, 42, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 629120, 42, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 629152, 42, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 200000, 64, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 629120, 64, kNnWave, 2, 4},
    {"DC_NN_SHARED=0", 629152, 64, kNnWave, 2, 4},
    {"DC_WAVES_PER_GROUP=2", 200000, 5, kNnWave, 6, 2},
    {"DC_WAVES_PER_GROUP=2", 629120, 5, kNnWave, 6, 2},
    {"DC_WAVES_PER_GROUP=2", 629152, 5, kNnWave, 6, 2},
    {"DC_WAVES_PER_GROUP=2", 200000, 10, kNnWave, 6, 2},
    {"DC_WAVES_PER_GROUP=2", 629120, 10, kNnWave, 6, 2},
    {"DC_WAVES_PER_GROUP=2", 629152, 10, kNnWave, 6, 2},
    {"DC_WAVES_PER_GROUP=2", 200000, 14, kNnWave, 4, 2},
    {"DC_WAVES_PER_GROUP=2", 629120, 14, kNnWave, 4, 2},
    {"DC_WAVES_PER_GROUP=2", 629152, 14, kNnWave, 4, 2},
    {"DC_WAVES_PER_GROUP=2", 200000, 26, kNnWave, 4, 2},
    {"DC_WAVES_PER_GROUP=2", 629120, 26, kNnWave, 4, 2},
    {"DC_WAVES_PER_GROUP=2", 629152, 26, kNnShared, 16, 4},
    {"DC_WAVES_PER_GROUP=2", 200000, 40, kNnWave, 2, 2},
    {"DC_WAVES_PER_GROUP=2", 629120, 40, kNnShared, 8, 4},
    {"DC_WAVES_PER_GROUP=2", 629152, 40, kNnShared, 8, 4},
    {"DC_WAVES_PER_GROUP=2", 200000, 42, kNnWave, 2, 2},
    {"DC_WAVES_PER_GROUP=2", 629120, 42, kNnShared, 8, 4},
    {"DC_WAVES_PER_GROUP=2", 629152, 42, kNnShared, 8, 4},
    {"DC_WAVES_PER_GROUP=2", 200000, 64, kNnWave, 2, 2},
    {"DC_WAVES_PER_GROUP=2", 629120, 64, kNnWave, 2, 2},
    {"DC_WAVES_PER_GROUP=2", 629152, 64, kNnWave, 2, 2},
};

static SweepSwitches switches_of(const char* sw) {
  SweepSwitches w;
  if (!strcmp(sw, "DC_POP_SHARED=1")) w.pop_shared = 1;
  if (!strcmp(sw, "DC_POP_SHARED=0")) w.pop_shared = 0;
  if (!strcmp(sw, "DC_NN_SHARED=1")) w.nn_shared = 1;
  if (!strcmp(sw, "DC_NN_SHARED=0")) w.nn_shared = 0;
  if (!strcmp(sw, "DC_POP_SYM=0")) w.pop_sym = false;
  if (!strcmp(sw, "DC_WAVES_PER_GROUP=2")) w.waves_per_group = 2;
  return w;
}

static int check_plans() {
  int bad = 0;
  for (const PopRow& r : kPopRows) {
    const PopPlan p = plan_pop(r.n_rows, r.n_cols, r.n_rad, r.kind, r.sink, switches_of(r.sw));
    const int nm = nm_for((int)r.n_cols);
    const bool ok = p.form == r.form && p.nr == r.nr && p.group_tiles == r.group_tiles && p.waves == r.waves &&
                    p.shift_steps == r.shift_steps && pop_form_built(p.form, nm) && p.pos_clean == (p.form == kPopWaveSym) &&
                    p.group_tiles == (p.form >= kPopShared ? 4u : 1u) * p.tq;
    if (!ok) {
      ++bad;
      fprintf(stderr, "plan_pop %s %u x %u, %d radii, kind %d, sink %d: form %d nr %d group %u waves %u shift %d\n", r.sw,
              r.n_rows, r.n_cols, r.n_rad, (int)r.kind, (int)r.sink, (int)p.form, p.nr, p.group_tiles, p.waves, p.shift_steps);
    }
  }
  for (const NnRow& r : kNnRows) {
    const NnPlan p = plan_nn(r.n_rows, r.n_cols, switches_of(r.sw));
    const bool ok = p.form == r.form && p.group_tiles == r.group_tiles && p.waves == r.waves &&
                    nn_form_built(p.form, nm_for((int)r.n_cols)) && p.coop_shares == kNnCoopMinShares;
    if (!ok) {
      ++bad;
      fprintf(stderr, "plan_nn %s %u x %u: form %d group %u waves %u\n", r.sw, r.n_rows, r.n_cols, (int)p.form,
              p.group_tiles, p.waves);
    }
  }
  return bad;
}

int main() {
  int bad = 0, cases = 0;
  const float Ms[] = {0.0f, 1e-30f, 3e-12f, 1e-4f, 0.37f, 1.3f, 5.0625f, 812.0f, 3e9f, 1e20f, 9e35f};
  const float r2s[] = {0.0f, 1e-38f, 1e-12f, 1e-4f, 0.01f, 0.04f, 0.36f, 2.25f, 1e4f, 1e30f, INFINITY};
  for (int D = 1; D <= 64; D += (D < 16 ? 1 : 7))
    for (float M : Ms)
      for (float r2 : r2s) {
        ++cases;
        const ScaleExp e = pick_scale_pop(M, r2, D);
        const double S = (double)e.c * (double)e.c;
        const double eps = guard_eps_pop(S * (double)M, S * (double)r2, D, e.g, e.a, e.rounded);
        bool ok = e.g == kMidShiftPop && e.a == kConstShiftPop && e.c > 0.0f && e.s2 == (float)S;
        if (e.rounded) {
          // the regular case: the band is at most 1 and the scale within a few percent of the largest such
          // (the sub-linear flush terms are the difference)
          ok = ok && eps <= 1.0 && eps > 0.95;
        } else {
          // the clamps: a power of two; admissible unless the radius is beyond every scale (then thr is capped)
          int ex = 0;
          ok = ok && frexpf(e.c, &ex) == 0.5f;
          if (r2 < INFINITY && M > 0.0f) ok = ok && eps <= 1.0;
        }
        if (eps <= 1.0) {
          // coordinates (A form, and -2x in the B form) and c_q / 2^a fit the fp16 range
          const double xa = sqrt(S * (double)M);
          const double cq = S * (double)M + fmin(S * (double)r2, (double)kThrCapPop) + 1.0;
          ok = ok && 2.0 * xa < 32768.0 && ldexp(cq, -e.a) < 65504.0 && ldexp(65504.0, e.a) > 4.0 * S * (double)M + 2.0;
        }
        if (!ok) {
          ++bad;
          fprintf(stderr, "D %d M %g r2 %g: c %g rounded %d eps %g\n", D, M, r2, e.c, e.rounded, eps);
        }
      }
  // pieces: v = hi + mid 2^-g + rho with |rho| <= max(2^-22 |v|, 2^(-14-g)); the hi 2^-g copy is exact or zero
  const Scale sc = make_scale(ScaleExp{181.0f, 32761.0f, kMidShiftPop, kConstShiftPop, 1});
  uint32_t seed = 12345u;
  for (int i = 0; i < 200000; ++i) {
    seed = seed * 1664525u + 1013904223u;
    const float mag = ldexpf(1.0f + (float)(seed >> 9) * (1.0f / 8388608.0f), (int)(seed % 37u) - 26);   // 2^-26 .. 2^11
    const float v = (seed & 0x100u) ? -mag : mag;
    const Pieces p = split2(v, sc.up, sc.dn);
    const double rec = (double)f16_val(p.hi) + (double)f16_val(p.mid) * (double)sc.dn;
    const double tol = fmax(ldexp(fabs((double)v), -22), ldexp(1.0, -14 - sc.g));
    const double hd = (double)f16_val(p.hi_dn), want = (double)f16_val(p.hi) * (double)sc.dn;
    if (fabs(rec - (double)v) > tol || !(hd == want || (hd == 0.0 && fabs(want) < ldexp(1.0, -14)))) {
      ++bad;
      if (bad < 20) fprintf(stderr, "split2(%g): hi %g mid %g hi_dn %g\n", v, f16_val(p.hi), f16_val(p.mid), f16_val(p.hi_dn));
    }
  }
  const int bad_plans = check_plans();
  printf("scale rule: %d cases, pieces: 200000 values, violations %d; plans: %zu rows, violations %d\n", cases, bad,
         sizeof(kPopRows) / sizeof(kPopRows[0]) + sizeof(kNnRows) / sizeof(kNnRows[0]), bad_plans);
  bad += bad_plans;
  printf("%s\n", bad ? "FAILED" : "OK");
  return bad ? 1 : 0;
}
