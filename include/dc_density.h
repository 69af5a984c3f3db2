/*
 * dc_density.h -- C ABI of the MI355X-native `clustering density` hot path.
 *
 * Drop-in boundary for moldyn/Clustering's GPU plug-in surface.  Every entry
 * point names the reference interface it replaces (paths relative to the
 * reference's src/).  The reference selects its GPU path at compile time
 * (-DUSE_CUDA) and calls the free functions of density_clustering_cuda.hpp; the
 * C++ shim in clustering_amd/csrc/density_clustering_hip.{hpp,cpp} re-creates
 * exactly those signatures (namespace Clustering::Density::CUDA) on top of this
 * C ABI.  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *   - plain C types only; no C++/torch types cross this boundary.
 *   - every function returns 0 on success or a negative dc_status; the message
 *     is available from dc_hip_last_error() (thread-local).  Nothing here prints
 *     or exits -- the C++ shim restores the reference's "message on stderr, then
 *     exit(EXIT_FAILURE)" convention (density_clustering_cuda.cu:21-30).
 *   - coords: row-major float32 [n_rows][n_cols], as read_coords() produces
 *     (tools.hxx:39-111).  Frame ids are 0-based.
 *   - populations are uint32 on the device like the reference's
 *     (density_clustering_cuda.cu:64,120), laid out radius-major
 *     pops[r*n_rows + i] (density_clustering_cuda.cu:130) IN THE ORDER OF THE
 *     radii ARGUMENT; rows outside [i_from, i_to) are written 0, so that
 *     per-device partials merge by summation (density_clustering_cuda.cu:171-180).
 *   - results follow the reference's OpenMP CPU path bit for bit (the parity
 *     target named by BASELINE.json; density_clustering.cpp:126-288):
 *       pop_r[i] = 1 + #{ j != i : d2(i,j) <  fl32(r*r) }      (strict)
 *       nn[i]    = lexicographic min over j != i of (d2(i,j), j)
 *       nn_hd[i] = same over { j : fe[j] < fe[i] }; empty -> (n_rows+1, FLT_MAX)
 *     with d2 in the reference binary's float summation order.
 *   - "_dev" functions take DEVICE pointers, run on the given hipStream_t
 *     (passed as void*; NULL = the default stream) and are asynchronous unless
 *     stated otherwise.  Functions without the suffix take HOST pointers, manage
 *     device memory themselves and are synchronous -- they mirror the
 *     reference's per-GPU host functions.
 */
#ifndef DC_DENSITY_H
#define DC_DENSITY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define DC_API __attribute__((visibility("default")))
#else
#define DC_API
#endif

typedef enum dc_status {
  DC_OK = 0,
  DC_ERR_INVALID_ARGUMENT = -1,
  DC_ERR_NO_DEVICE = -2,      /* reference: "no CUDA-compatible GPUs found", cuda.cu:37-40 */
  DC_ERR_HIP = -3,            /* a HIP runtime call failed; see dc_hip_last_error() */
  DC_ERR_TOO_LARGE = -4,      /* n_rows + 1 does not fit the uint32 index type, or n_cols > 2^32 - 65 */
  DC_ERR_WORKSPACE = -5       /* workspace missing or too small */
} dc_status;

/* kernel family selector for the two pairwise sweeps */
typedef enum dc_variant {
  DC_VARIANT_AUTO = 0,        /* fastest available: pruned MFMA when n_cols allows, else direct */
  DC_VARIANT_DIRECT = 1,      /* VALU, direct differences in the canonical order: exact by construction */
  DC_VARIANT_MFMA = 2,        /* matrix-core Gram form (two fp16 pieces per coordinate, n_cols <= 64) as a
                                 classifier + guard band + canonical re-check; every pair evaluated */
  DC_VARIANT_MFMA_PRUNED = 3, /* the same on spatially ordered frames, skipping tile pairs farther apart than
                                 the radius (the GPU counterpart of the reference's box grid,
                                 density_clustering.cpp:41-89); identical results */
  DC_VARIANT_MFMA32 = 4,      /* the literal fp32-input MFMA (v_mfma_f32_32x32x2_f32) Gram form, every pair evaluated:
                                 the instance BASELINE's "fraction of the fp32 MFMA roofline" is quoted on; n_cols
                                 9..10 only, one radius per sweep; identical results (classifier + band + re-check).
                                 The same kernels for 1..32 columns and several radii per sweep: the entry points
                                 dc_hip_populations_fp32_dev / dc_hip_nearest_neighbors_fp32_dev below */
  DC_VARIANT_CROSS_PRUNED = 5 /* populations of new frames against a reference on the matrix cores with tile-pair
                                 pruning: both sets ordered by the cells of one grid on columns 0/1, tile pairs at
                                 least the largest radius apart skipped; n_cols <= 64; identical results.  ONLY
                                 dc_hip_populations_cross_dev takes it: every other entry point refuses it */
} dc_variant;
/* may be OR-ed into the `variant` argument of the _dev sweeps: the column means, max |x - mean|^2, the
 * non-finite flag and the bounding box in this workspace's header were computed by an earlier sweep over
 * the SAME d_coords (same contents) and are still valid -- the sweep skips its three statistics passes.
 * The reference runs populations and then neighbours over one coordinate array
 * (density_clustering.cpp:616-621, 659-663): the second call of such a pair may set it.  The claim is
 * CHECKED on the device: address, shape and a 64-bit content fingerprint of the whole array (one streaming
 * pass, recomputed by the claiming call) must equal what the statistics pass stored; otherwise -- another
 * array, the same buffer rewritten in place, a reused allocation -- the sweep is answered by the exact
 * direct kernels: slower, same results. */
#define DC_FLAG_STATS_VALID 0x100
#define DC_VARIANT_MASK 0xFF

/* message of the last failing call on this thread ("" if none). */
DC_API const char* dc_hip_last_error(void);

/* library/ABI version, bumped on any change of a signature or of a documented contract.  Hosts check it at
 * load time (clustering_amd/capi.py, density_clustering_hip.cpp).
 *   1  rounds 1-2 up to the sessions
 *   2  sessions (dc_hip_session_*), segment entry points whose populations are PARTIAL counts of ALL rows
 *      (symmetric one-radius sweeps credit both frames of a pair), dc_hip_session_merge_mode, host-merge
 *      fallback, DC_FLAG_STATS_VALID
 *   3  dc_hip_session_merge_note (which merge a multi-device session runs, and why),
 *      dc_hip_workspace_mfma_counters_dev, dc_hip_workspace_layout_status_dev
 *   4  dc_hip_build_digest (which sources this binary was built from)
 *   5  dc_hip_canon_order (which summation order of the reference's distance loop this binary reproduces) */
#define DC_HIP_ABI_VERSION 5
DC_API int dc_hip_abi_version(void);

/* digest of the sources this library was built from (clustering_amd/csrc + include/, comments left out:
 * clustering_amd/csrc/digest.py; 16 hex digits, embedded by the Makefile).  What a measurement is tied to: bench.py
 * prints it as "library_digest" and refuses counter profiles (profiles/ *_pmc.json) taken on another one. */
DC_API const char* dc_hip_build_digest(void);

/* The summation order of the canonical squared distance this library was built for: "sse2" -- the reference's DEFAULT
 * build (density_clustering.cpp:171-176, 263-268 under CMakeLists.txt:37-45: four lane sums, a pair tail) -- or "avx" --
 * a reference built with -DCPU_ACCELERATION=AVX (CMakeLists.txt:73-76: eight lane sums, a four-column step, scalar tails).
 * Integer results are bit-exact against the reference build of the SAME order; the two orders differ in the last bit of
 * some distances, i.e. in a few frames on a radius.  `make -C clustering_amd/csrc CANON=avx` builds the other library
 * into clustering_amd/lib_avx/ (same file name, same ABI). */
DC_API const char* dc_hip_canon_order(void);

/* replaces Clustering::Density::CUDA::get_num_gpus() (density_clustering_cuda.hpp:16-17,
 * density_clustering_cuda.cu:32-43).  Returns the device count (>= 0) or a negative status;
 * 0 devices is NOT an error here (the C++ shim turns it into the reference's exit). */
DC_API int dc_hip_device_count(void);

/* ---------------------------------------------------------------------------------------
 * device-pointer entry points (inputs already resident in HBM)
 * ------------------------------------------------------------------------------------- */

/* bytes of scratch the _dev sweeps may need for this problem size (MFMA operand images,
 * norms; 0-filled by the callee as needed).  Pass a buffer at least this large. */
DC_API size_t dc_hip_workspace_bytes(size_t n_rows, size_t n_cols, size_t n_radii);

/* statistics of the sweeps that last ran in this workspace (asynchronous pruned variants leave them
 * in the workspace header): number of 32x32 frame-pair tiles actually evaluated by the population
 * and by the neighbour sweep (every pair = n_rows^2/1024 per full sweep; the direct kernels and
 * DC_VARIANT_MFMA do not count and report 0).  Synchronises the stream. */
DC_API int dc_hip_workspace_counters_dev(const void* d_workspace, uint64_t* pop_tiles,
                                         uint64_t* nn_tiles, void* stream);
/* ... and the matrix-core instructions (v_mfma_f32_32x32x16_f16: 32*32*16*2 flop each) those sweeps ISSUED, counted by the
 * kernels themselves: tiles x MFMAs per chain for the population sweeps, fewer for the neighbour sweeps, whose chains
 * mostly stop after their coarse MFMAs (the executed-flop figure of bench.py's roofline; it equals
 * SQ_VALU_MFMA_BUSY_CYCLES / 32 of a counter profile).  Synchronises the stream. */
DC_API int dc_hip_workspace_mfma_counters_dev(const void* d_workspace, uint64_t* pop_mfma, uint64_t* nn_mfma,
                                              void* stream);

/* diagnostics of the last pruned POPULATION sweep that ran in this workspace (same n_rows, n_cols): the number of
 * components the frames were cut into (sets at least r_max apart in columns 0/1, each measured from its own origin by
 * the matrix-core sweep; 1 = one origin, the column means), the global max |x - mean|^2, the bound of
 * max |x - origin(component of x)|^2 that the sweep's guard band follows, and the scale S of that sweep (band = 1 / S in
 * the units of d2).  Synchronises the stream. */
DC_API int dc_hip_workspace_components_dev(const void* d_workspace, size_t n_rows, size_t n_cols,
                                          uint32_t* n_components, float* extent2_global, float* extent2_local,
                                          float* scale, void* stream);

/* measurement aid (bench.py's roofline entry): with timing enabled the library brackets its MAIN sweep
 * kernels (population_count / nearest_neighbor_search counterparts) with HIP events on the launch stream;
 * dc_hip_last_sweep_ms returns the duration of the kernels of one kind (0 population, 1 neighbour) launched on
 * the calling thread's current device since the previous read -- the sweep kernel alone, without the ordering /
 * operand-image passes of the call.  Synchronises on the kernel's end.  Returns DC_ERR_INVALID_ARGUMENT if no
 * sweep of that kind was recorded. */
DC_API int dc_hip_sweep_timing(int enable);
DC_API int dc_hip_last_sweep_ms(int kind, float* ms);

/* replaces the kernel loop of calculate_populations_per_gpu (density_clustering_cuda.cu:45-137;
 * kernel population_count, density_clustering_cuda_kernels.cu:9-56): ONE launch sweeps all
 * n_rows reference frames for the query rows [i_from, i_to).
 *   d_coords  [n_rows*n_cols] float32, device
 *   radii     [n_radii] float32, HOST (tiny; the reference also passes them from the host)
 *   d_pops    [n_radii*n_rows] uint32, device, fully overwritten (0 outside the row range) */
DC_API int dc_hip_populations_dev(const float* d_coords, size_t n_rows, size_t n_cols,
                                  const float* radii, size_t n_radii, size_t i_from, size_t i_to,
                                  uint32_t* d_pops, void* d_workspace, size_t workspace_bytes,
                                  int variant, void* stream);

/* The same sweep for one SEGMENT of a sharded run instead of a row range: rank `segment` of
 * `n_segments` (density_clustering_cuda.cu:149-169 gives every GPU a contiguous block of rows; any
 * partition serves, as long as the partial results merge).  With the pruned matrix-core sweep a
 * segment is every n_segments-th query group of the SPATIAL order (128 - 192 frames of one grid cell):
 * a rank's queries are as compact as those of a full sweep and prune as well (a block of consecutive
 * rows of a trajectory is spread over the whole conformational space), and dealing the groups out
 * cyclically gives every rank the same mix of dense and sparse regions; with every other variant,
 * n_cols > 64 or non-finite data the
 * segment is the reference's row block.  d_pops: PARTIAL populations that merge by summation over the
 * segments (the reference merges its per-GPU partials the same way, density_clustering_cuda.cu:171-180).
 * A one-radius pruned sweep evaluates every pair of query groups once and credits both frames
 * (d2(i,j) = d2(j,i), the reference's own i < j loop, density_clustering.cpp:170-182), so a segment's
 * counts cover all rows; the other sweeps write the final counts of the segment's own rows and zeros
 * elsewhere.  Only the sum over all segments is a population. */
DC_API int dc_hip_populations_segment_dev(const float* d_coords, size_t n_rows, size_t n_cols,
                                          const float* radii, size_t n_radii, size_t segment,
                                          size_t n_segments, uint32_t* d_pops, void* d_workspace,
                                          size_t workspace_bytes, int variant, void* stream);

/* replaces Clustering::Density::calculate_free_energies (density_clustering.cpp:197-212), which the
 * reference runs on the host in both builds.  fe[i] = (float)-log((double)((float)pop[i] * (1.0f/max)))
 * -- with the reference's bits: the device evaluates the double log, and every row whose value lies
 * within 64 ulp(double) of a float rounding boundary (where a few ulp of difference between two libms
 * could show) is recomputed by the HOST libm.  Synchronises the stream once (reads max_pop).
 *   d_pops [n_rows] uint32 device (one radius), d_fe [n_rows] float32 device.
 * max_pop_out (optional, host) receives the maximum population. */
DC_API int dc_hip_free_energies_dev(const uint32_t* d_pops, size_t n_rows, float* d_fe,
                                    uint32_t* max_pop_out, void* stream);

/* replaces the kernel loop of nearest_neighbors_per_gpu (density_clustering_cuda.cu:184-284; kernel
 * nearest_neighbor_search, density_clustering_cuda_kernels.cu:58-130) for query rows [i_from, i_to).
 *   d_fe      [n_rows] float32 device
 *   d_nn_idx / d_hd_idx [n_rows] uint32, d_nn_d2 / d_hd_d2 [n_rows] float32, device; rows outside the
 *   range are written with the "none" value (n_rows+1, FLT_MAX) of density_clustering.cpp:242-245. */
DC_API int dc_hip_nearest_neighbors_dev(const float* d_coords, size_t n_rows, size_t n_cols,
                                        const float* d_fe, size_t i_from, size_t i_to,
                                        uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                        float* d_hd_d2, void* d_workspace, size_t workspace_bytes,
                                        int variant, void* stream);

/* neighbour sweep for one segment of a sharded run (see dc_hip_populations_segment_dev); rows of other
 * segments hold (n_rows+1, FLT_MAX), so partials merge by taking, per row, the minimum of
 * (d2 bits << 32 | index) -- only the owner's value is smaller than the "none" value. */
DC_API int dc_hip_nearest_neighbors_segment_dev(const float* d_coords, size_t n_rows, size_t n_cols,
                                                const float* d_fe, size_t segment, size_t n_segments,
                                                uint32_t* d_nn_idx, float* d_nn_d2,
                                                uint32_t* d_hd_idx, float* d_hd_d2,
                                                void* d_workspace, size_t workspace_bytes,
                                                int variant, void* stream);

/* Merging the neighbour partials of a sharded run (density_clustering_cuda.cu:311-326 overwrites row by
 * row on the host): [2][n_rows] order-preserving 64-bit words (d2 bits << 32 | index) -- nn first, then
 * nn_hd.  d2 >= 0, so the words of a row order like the lexicographic (d2, index): the owner's word is
 * the minimum over the ranks (everybody else holds the "none" value (n_rows+1, FLT_MAX)), i.e. ONE
 * all-reduce(min) of int64 merges all four arrays. */
DC_API int dc_hip_neighbors_pack_dev(const uint32_t* d_nn_idx, const float* d_nn_d2,
                                     const uint32_t* d_hd_idx, const float* d_hd_d2, size_t n_rows,
                                     unsigned long long* d_words, void* stream);
DC_API int dc_hip_neighbors_unpack_dev(const unsigned long long* d_words, size_t n_rows,
                                       uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                       float* d_hd_d2, void* stream);

/* The same merge as an ALL-GATHER (half the bytes, no reduction): every rank compacts the results of its own
 * segment's rows into a dense block [4][block_rows] uint32 (nn_idx, nn_d2 bits, hd_idx, hd_d2 bits, by local
 * position in the segment; pad entries hold the "none" value), the blocks of all ranks are gathered into
 * [n_segments][4][block_rows], and the gathered blocks are scattered back to the four arrays by frame.
 * With the pruned matrix-core sweep a segment is every n_segments-th query group of the sweep's spatial order,
 * which every rank derives identically from the replicated coordinates and free energies: pack and unpack read
 * the ordering that dc_hip_nearest_neighbors_segment_dev left in THIS rank's workspace (same n_rows, n_cols,
 * variant; no other sweep in between).  Otherwise (other variants, n_cols > 64, flagged data) the blocks are the
 * reference's row blocks (density_clustering_cuda.cu:293, 305-308, 311-326). */
DC_API size_t dc_hip_neighbors_block_rows(size_t n_rows, size_t n_cols, size_t n_segments);
DC_API int dc_hip_neighbors_block_pack_dev(const uint32_t* d_nn_idx, const float* d_nn_d2,
                                           const uint32_t* d_hd_idx, const float* d_hd_d2, size_t n_rows,
                                           size_t n_cols, size_t segment, size_t n_segments,
                                           const void* d_workspace, size_t workspace_bytes, int variant,
                                           uint32_t* d_block, void* stream);
DC_API int dc_hip_neighbors_block_unpack_dev(const uint32_t* d_blocks, size_t n_rows, size_t n_cols,
                                             size_t n_segments, const void* d_workspace,
                                             size_t workspace_bytes, int variant, uint32_t* d_nn_idx,
                                             float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* stream);
/* The unpack compares the layout headers of the gathered blocks ON THE DEVICE before it scatters anything: on a mismatch
 * (a rank derived another order) NOTHING is written -- the output arrays keep whatever they held -- and a word of the
 * workspace header records the verdict of THAT unpack (pruned variants only; with any other variant the workspace is not
 * touched and the host compares the headers itself).  The word describes the LAST unpack only: the next unpack, and the
 * preparation of the next sweep in the workspace, overwrite it.  This call reads it (synchronises the stream): *mismatch =
 * 1 if the last unpack refused its blocks.  A host that wants every step covered asks after every step, before the next
 * call into the workspace (clustering_amd.distributed does unless told otherwise; bench.py asks after its instrumented
 * steps and after the last timed one). */
DC_API int dc_hip_workspace_layout_status_dev(const void* d_workspace, int* mismatch, void* stream);

/* replaces Clustering::Density::compute_sigma2 (density_clustering.cpp:334-343): mean of the nearest-
 * neighbour d2 accumulated in double IN FRAME ORDER (bit-stable), on the device (one block, fixed
 * reduction tree would change bits -- so this is a single ordered pass over a device->host copy).
 * Synchronises the stream. */
DC_API int dc_hip_sigma2_dev(const float* d_nn_d2, size_t n_rows, double* sigma2_out, void* stream);

/* the radius graph that the reference's screening walks one frame at a time: replaces the O(n^2) scans
 * of high_density_neighborhood (density_clustering.cpp:292-332, called per frame from
 * density_clustering_common.cpp:97-121; CUDA: density_clustering_cuda.cu:396-594) by ONE sweep that
 * lists every unordered frame pair {i, j}, i != j, whose canonical d2 is < r2 (strict, :319).  The
 * pruned matrix-core sweep for n_cols <= 64; an exact direct sweep over all pairs for any wider rows
 * and for coordinates that are not finite (inf / NaN in a row: no partners, population 1, as in the
 * reference), chosen on the device like the populations' fallback.
 *   r2       the squared distance itself (the reference passes max_dist = 4*sigma2, a float); a NaN, like 0 or a
 *            negative value, holds no pair
 *   d_pops   [n_rows] uint32 device, out: populations at that radius (1 + number of partners)
 *   d_pairs  [capacity][2] uint32 device, out: frame ids of the pairs, in no particular order, each
 *            pair once; may be NULL with capacity 0 to count only
 *   d_count  device uint64, out: number of pairs found -- if it exceeds capacity only the first
 *            `capacity` were written (call again with a larger buffer).
 * Needs a workspace as above for n_cols <= 64; for n_cols > 64 none (NULL / 0: dc_hip_workspace_bytes is 0) -- this
 * call runs the direct sweep there; for 65..256 columns dc_hip_radius_pairs_wide_dev below is the matrix-core form. */
DC_API int dc_hip_radius_pairs_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                   uint32_t* d_pops, uint32_t* d_pairs, size_t capacity,
                                   unsigned long long* d_count, void* d_workspace,
                                   size_t workspace_bytes, void* stream);

/* one Boruvka round on that radius graph, for screenings that only need its CONNECTIVITY below a
 * free-energy threshold (density_clustering_common.cpp:37-134 started from an empty clustering): for
 * every component the lightest pair that leaves it.  No pair list is materialised.
 *   d_comp   [n_rows] uint32 device: component id of every frame (the id is any frame id < n_rows)
 *   d_rank   [n_rows] uint32 device: a permutation of 0..n_rows-1 (position in order of free energy);
 *            the weight of a pair is (max(rank), min(rank)), compared lexicographically
 *   d_best   [n_rows] uint64 device, out: d_best[id] = (max << 32 | min) of the lightest pair with
 *            canonical d2 < r2 that joins component id to another one, ~0 if there is none
 *   d_pops   [n_rows] uint32 device, out: populations at that radius
 * Needs n_rows <= 2^24 - 32768 (the sweep's queue holds 24-bit positions of the padded spatial order; more rows are
 * DC_ERR_INVALID_ARGUMENT), and a workspace as above for n_cols <= 64 (none for n_cols > 64).  Any column
 * count and coordinates that are not finite are served (the direct sweep, as for the pairs). */
DC_API int dc_hip_radius_min_edge_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                      const uint32_t* d_comp, const uint32_t* d_rank,
                                      unsigned long long* d_best, uint32_t* d_pops, void* d_workspace,
                                      size_t workspace_bytes, void* stream);
/* the same for one segment of a sharded run (n_segments > 0): only the pairs seen from the queries of
 * that segment enter d_best (every pair is seen from both of its ends, possibly by different segments);
 * the partial d_best arrays merge by an element-wise UNSIGNED minimum, the partial d_pops by summation.
 * The segments are those of the pruned sweep's spatial order; for n_cols > 64 or non-finite data they
 * are the reference's row blocks (density_clustering_cuda.cu:149,165-169) -- either is a partition. */
DC_API int dc_hip_radius_min_edge_segment_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                              const uint32_t* d_comp, const uint32_t* d_rank,
                                              size_t segment, size_t n_segments,
                                              unsigned long long* d_best, uint32_t* d_pops,
                                              void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * cross sweeps: new frames measured against a reference trajectory (no counterpart in the reference, whose
 * sweeps are all self-sweeps; the same arithmetic and decision rules as those)
 * -------------------------------------------------------------------------------------
 * Inputs: d_query [n_query][n_cols] and d_ref [n_ref][n_cols], float32 row-major, the same n_cols >= 1 (any width);
 * d_query == d_ref is allowed.  Only the query rows [i_from, i_to) are answered.  d2(q, j) is the canonical squared
 * distance of this build's summation order; it is bitwise symmetric in its two rows.
 *   pop_r[q] = #{ j in [0, n_ref) : d2(Q_q, R_j) < fl32(r*r) }    -- NO self term
 *       [n_radii][n_query] in the order of the radii argument, 0 outside the row range.  With Q bit-identical to R,
 *       r > 0 and finite rows this equals the self-sweep populations exactly (the self pair supplies the "+1"): a
 *       copy of reference frame j gets exactly pop_R(j).
 *   nn[q]    = lexicographic minimum of (d2, j) over ALL j (no exclusion: a duplicate gives d2 = 0), among the
 *              candidates with d2 < FLT_MAX (the reference's strict test against its initial value)
 *   nn_hd[q] = the same over { j : fe_ref[j] < fe_query[q] } (IEEE comparison: a NaN is never lower and has no lower
 *              neighbour, -0.0 is not lower than +0.0).  With Q = R[S] and fe_query = fe_ref[S] it equals the
 *              self-sweep nn_hd of the rows S bit for bit (a frame is not lower than itself).
 *   no candidate: (n_ref + 1, FLT_MAX); rows outside the range hold that value too.
 * A non-finite row (inf / NaN in Q or in R) has no partners: it adds 0 to every population and is never a neighbour.
 * Sizes: n_ref + 1 and n_query must fit uint32 (else DC_ERR_TOO_LARGE).
 * Variants: DC_VARIANT_AUTO (the matrix-core sweep for n_cols <= 64 and finite data -- chosen on the device, like the
 * self sweeps' fallback -- the direct kernels otherwise), DC_VARIANT_DIRECT, DC_VARIANT_MFMA (n_cols <= 64 only; every
 * pair, one origin and one scale over Q and R together), and -- dc_hip_populations_cross_dev only --
 * DC_VARIANT_CROSS_PRUNED (n_cols <= 64 only: the same origin, scale and arithmetic on both sets ordered by one cell
 * grid, tile pairs farther apart than the call's largest radius skipped; it needs the larger workspace of
 * dc_hip_cross_workspace_bytes_for, and leaves its evaluated 32x32 tile pairs and issued MFMAs where
 * dc_hip_workspace_counters_dev / dc_hip_workspace_mfma_counters_dev read them; a reference of more than 2^24 rows is
 * answered by the every-pair sweep in the same workspace).  DC_VARIANT_MFMA_PRUNED, DC_VARIANT_MFMA32 and
 * DC_FLAG_STATS_VALID are still refused (DC_ERR_INVALID_ARGUMENT): the self sweeps' pruned variant means components,
 * a symmetric form and statistics kept across calls, none of which a rectangle has -- the pruned cross sweep is a
 * sweep of its own and has a value of its own.  DC_VARIANT_AUTO chooses what it chose before that value existed.
 * Results are the same for every variant. */

/* bytes of scratch the cross sweeps need (0 when n_cols > 64: the direct kernels need none) */
DC_API size_t dc_hip_cross_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols);
/* ... for one variant: what dc_hip_cross_workspace_bytes returns for DC_VARIANT_AUTO / _DIRECT / _MFMA, the larger
 * pruned layout for DC_VARIANT_CROSS_PRUNED (a smaller workspace: DC_ERR_WORKSPACE), 0 when n_cols > 64 and for a
 * variant the cross sweeps refuse */
DC_API size_t dc_hip_cross_workspace_bytes_for(size_t n_query, size_t n_ref, size_t n_cols, int variant);

/* populations of the query rows against the reference frames.  radii HOST [n_radii]; d_pops [n_radii][n_query]
 * device, fully overwritten. */
DC_API int dc_hip_populations_cross_dev(const float* d_query, size_t n_query, const float* d_ref, size_t n_ref,
                                        size_t n_cols, const float* radii, size_t n_radii, size_t i_from, size_t i_to,
                                        uint32_t* d_pops, void* d_ws, size_t ws_bytes, int variant, void* stream);

/* nearest reference frame, and nearest reference frame of strictly lower free energy.  d_fe_query [n_query],
 * d_fe_ref [n_ref] device; d_fe_query == NULL: nn only (d_fe_ref, d_hd_idx, d_hd_d2 may be NULL and are not written).
 * Outputs [n_query] device. */
DC_API int dc_hip_nearest_neighbors_cross_dev(const float* d_query, size_t n_query, const float* d_ref, size_t n_ref,
                                              size_t n_cols, const float* d_fe_query, const float* d_fe_ref,
                                              size_t i_from, size_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
                                              uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, size_t ws_bytes,
                                              int variant, void* stream);

/* The neighbour sweep with tile-pair pruning: an entry point of its own (no variant value: the variant argument of
 * dc_hip_nearest_neighbors_cross_dev keeps refusing DC_VARIANT_CROSS_PRUNED).  Same pointers, outputs and contract as
 * dc_hip_nearest_neighbors_cross_dev -- results are bit-identical to its DC_VARIANT_DIRECT -- for n_cols <= 64 only
 * (more: DC_ERR_INVALID_ARGUMENT, like DC_VARIANT_MFMA).  Both sets are ordered by the cells of one grid on columns 0/1,
 * the reference inside a cell by free energy; a query group visits the reference's 32-frame tiles in rings of growing
 * box distance and stops when the exact incumbents of all its queries lie inside the last ring, so tile pairs that
 * cannot matter are never evaluated.  Answered exactly as the other cross sweeps answer them, with all counters 0:
 * flagged data (a non-finite or overflowing row in either set, a NaN in fe_ref: the direct kernel, chosen on the
 * device), a reference of more than 2^24 positions (the every-pair matrix-core sweep in the same workspace),
 * n_ref == 0 or an empty row range ("none" everywhere).
 * Workspace: dc_hip_nearest_cross_pruned_workspace_bytes -- 0 for n_cols > 64, otherwise at least
 * dc_hip_cross_workspace_bytes of the same shape and monotone in either row count; smaller: DC_ERR_WORKSPACE. */
DC_API size_t dc_hip_nearest_cross_pruned_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols);
DC_API int dc_hip_nearest_neighbors_cross_pruned_dev(const float* d_query, size_t n_query, const float* d_ref,
                                                     size_t n_ref, size_t n_cols, const float* d_fe_query,
                                                     const float* d_fe_ref, size_t i_from, size_t i_to,
                                                     uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                                     float* d_hd_d2, void* d_ws, size_t ws_bytes, void* stream);
/* the last dc_hip_nearest_neighbors_cross_pruned_dev call in that workspace: 32x32 tile pairs evaluated, MFMA
 * instructions issued, reference shares of the launch; all 0 when the pruned kernel did not answer.  Any pointer may
 * be NULL.  Synchronises the stream. */
DC_API int dc_hip_nearest_cross_pruned_info_dev(const void* d_ws, uint64_t* nn_tiles, uint64_t* nn_mfma,
                                                uint32_t* n_shares, void* stream);

/* ---- ... and a RESIDENT REFERENCE for the two pruned cross sweeps (1..64 columns) ---------------------------------------
 * DC_VARIANT_CROSS_PRUNED of dc_hip_populations_cross_dev and dc_hip_nearest_neighbors_cross_pruned_dev for a caller who
 * streams batches of queries against ONE reference: the reference is prepared once, when it is opened -- origin, both
 * scales, grid, and per sweep its order, its gathered rows, boxes and operand image --, and a batch pays for itself alone.
 * The statistics cannot depend on a batch: the origin is the column mean of the reference, the grid its extent in columns
 * 0 / 1 (a query outside it lands in an edge cell; its tile's box is still formed from its own floats), and the scales are
 * those of FOUR TIMES the reference's largest |x - mean|^2: a query up to twice as far from the origin as the farthest
 * reference frame runs on the matrix cores.
 * The handle is a small host object.  It BORROWS d_ref and d_ws until it is closed, and d_query from
 * dc_hip_reference_stage_dev until the last sweep of that batch: all must stay valid and unchanged for that long.
 * d_fe_ref and d_fe_query are read by the call they are given to and not kept.  Calls on one handle are ordered by the
 * caller: on one stream, or with synchronisation between them.  Nothing here synchronises with the host but the two readers.
 *   workspace_bytes  a region sized by (n_ref, n_cols) that stays, one sized by (max_batch, n_cols) that a batch
 *                    rewrites, and the sort's scratch; 0 outside 1..64 columns or for a zero count; monotone in each argument
 *   open             prepares the reference (the population side once per handle: `reference_preparations` of the info
 *                    call counts its runs).  max_radius: the largest radius any population call on this handle will use,
 *                    any number >= 0, +inf allowed; the population scale -- and the resident operand image -- are those
 *                    of fl32(max_radius^2).  The neighbour side of the reference is prepared in its form without free energies
 *   set_free_energies  fe_ref[n_ref], as dc_hip_nearest_neighbors_cross_dev takes it: a copy by row is kept, and the
 *                    neighbour side of the reference is prepared again, ordered by (cell, free energy); may be called
 *                    again with new values
 *   stage            the batch: ONE pass over its rows (the gate, and the cell keys on both grids), then per sweep its
 *                    order, boxes and operand image.  n_query <= max_batch; n_query == 0 stages an empty batch, whose
 *                    sweeps return DC_OK and write nothing
 *   populations      d_pops[n_radii][n_query] = dc_hip_populations_cross_dev's over the whole batch, bit for bit: strict <,
 *                    no self term, radii (host pointer) in any order.  A radius whose fl32(r * r) exceeds fl32(max_radius^2)
 *                    is refused before the device is touched
 *   nearest          the four arrays of dc_hip_nearest_neighbors_cross_dev over the whole batch, bit for bit: the least
 *                    (d2, ROW of R); "none" = (n_ref + 1, FLT_MAX); d_fe_query == NULL: nn only, the hd outputs may be NULL
 *                    and are not written
 * The two sweeps of a staged batch run in either order and any number of times without a second preparation.
 * Flagged data is answered by the direct kernels behind the device-side gate, without a host synchronisation, with the
 * same results; the counters then read zero.  `answered` of the info call says who answered the LAST sweep:
 *   0 the matrix cores;  1 the direct kernels, the reference holds a non-finite or overflow-prone row;  2 the direct
 *   kernels, the staged batch holds a row that is non-finite or farther from the origin than the scales allow;  3 the
 *   direct kernel, a NaN in fe_ref or in d_fe_query (the neighbour sweep with free energies only: populations, and
 *   neighbours without free energies, stay on the matrix cores).
 * A flag lasts as long as what raised it: the batch's until the next stage, the free energies' until they are set again
 * (fe_ref) or until the next neighbour sweep (d_fe_query).
 * info (tiles: 32x32 tile pairs evaluated, mfmas: MFMA instructions issued, shares: the reference shares of a neighbour
 * sweep's launch, 0 after a population sweep -- all of the last sweep; any pointer may be NULL) and order (which: 0 the
 * population sweep's orders, 1 the neighbour sweep's; d_perm_q[n_query of the staged batch], d_perm_r[n_ref], position ->
 * row; either may be NULL) SYNCHRONISE.
 * Refusals, all before a device is touched, dc_hip_last_error names the function: n_cols outside 1..64, n_ref == 0,
 * max_batch == 0, a max_radius that is NaN or negative, a NULL array, handle or `out`, n_query > max_batch, a sweep before
 * any stage, d_fe_query before free energies were set, a radius beyond max_radius, `which` other than 0 / 1:
 * DC_ERR_INVALID_ARGUMENT; n_ref + 1 or max_batch beyond uint32, either count times n_cols beyond the element arithmetic
 * (as the cross calls check them), or a reference whose padded order exceeds 2^24 positions (the per-call entry points
 * keep serving it): DC_ERR_TOO_LARGE; a workspace smaller than dc_hip_reference_workspace_bytes, or none:
 * DC_ERR_WORKSPACE.  On a refusal of open *out is NULL. */
typedef struct dc_reference dc_reference;
DC_API size_t dc_hip_reference_workspace_bytes(size_t n_ref, size_t n_cols, size_t max_batch);
DC_API int dc_hip_reference_open_dev(const float* d_ref, size_t n_ref, size_t n_cols, size_t max_batch, float max_radius,
                                     void* d_ws, size_t ws_bytes, void* stream, dc_reference** out);
DC_API void dc_hip_reference_close(dc_reference* reference);
DC_API int dc_hip_reference_set_free_energies_dev(dc_reference* reference, const float* d_fe_ref, void* stream);
DC_API int dc_hip_reference_stage_dev(dc_reference* reference, const float* d_query, size_t n_query, void* stream);
DC_API int dc_hip_reference_populations_dev(dc_reference* reference, const float* radii, size_t n_radii, uint32_t* d_pops,
                                            void* stream);
DC_API int dc_hip_reference_nearest_dev(dc_reference* reference, const float* d_fe_query, uint32_t* d_nn_idx, float* d_nn_d2,
                                        uint32_t* d_hd_idx, float* d_hd_d2, void* stream);
DC_API int dc_hip_reference_info_dev(dc_reference* reference, uint64_t* tiles, uint64_t* mfmas, uint32_t* shares,
                                     uint32_t* answered, uint32_t* reference_preparations, void* stream);
DC_API int dc_hip_reference_order_dev(dc_reference* reference, int which, uint32_t* d_perm_q, uint32_t* d_perm_r, void* stream);

/* ---- matrix-core sweeps for rows of 65..256 columns ("wide" sweeps) ----------------------------------------------
 * Every-pair self sweeps on the f16 matrix cores whose K axis streams through LDS, with the results of
 * dc_hip_populations_dev / dc_hip_nearest_neighbors_dev bit for bit (classifier + guard band + canonical re-check;
 * flagged data -- a non-finite or overflow-prone row, a NaN free energy -- is answered by the direct kernels behind
 * a device-side gate).  Entry points of their own: no dc_variant value selects them, DC_VARIANT_AUTO / _MFMA keep
 * sending rows wider than 64 columns to the direct kernels.
 * Contracts as for the two sweeps above: outputs fully overwritten, 0 / "none" = (n_rows + 1, FLT_MAX) outside
 * [i_from, i_to); radii in any order, one matrix-core chain per tile pair for up to 8 radii of a call.
 * n_cols outside 65..256: DC_ERR_INVALID_ARGUMENT; a workspace smaller than dc_hip_wide_workspace_bytes:
 * DC_ERR_WORKSPACE; sizes: DC_ERR_TOO_LARGE as above; n_rows == 0 or an empty range: DC_OK.
 * dc_hip_wide_workspace_bytes: 0 outside 65..256 columns (and for no rows), monotone in n_rows. */
DC_API size_t dc_hip_wide_workspace_bytes(size_t n_rows, size_t n_cols, size_t n_radii);
DC_API int dc_hip_populations_wide_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* radii,
                                       size_t n_radii, size_t i_from, size_t i_to, uint32_t* d_pops, void* d_ws,
                                       size_t ws_bytes, void* stream);
DC_API int dc_hip_nearest_neighbors_wide_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* d_fe,
                                             size_t i_from, size_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
                                             uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, size_t ws_bytes,
                                             void* stream);
/* ---- the fp32-input matrix-core sweeps for rows of 1..32 columns ("fp32" sweeps) ----------------------------------
 * DC_VARIANT_MFMA32's kernels (v_mfma_f32_32x32x2_f32, every pair evaluated, classifier + band + canonical re-check)
 * for every width the fp32 image fits the workspace of dc_hip_workspace_bytes, and with up to 8 radii of a call sharing
 * ONE pass of the MFMAs: ceil(n_cols / 2) K-steps (at some widths one zero step more: dc_hip_fp32_plan), the image
 * scaled for the call's largest radius, the per-chain tile test against that radius, the two-bit strings and the band
 * re-check per radius.  Results: those of dc_hip_populations_dev / dc_hip_nearest_neighbors_dev bit for bit.  Entry
 * points of their own: no dc_variant value selects them, DC_VARIANT_MFMA32 keeps serving 9..10 columns only.
 *   dc_hip_populations_fp32_dev        replaces density_clustering_cuda.cu:45-137 (the radius loop of :112-131 inside
 *                                      one sweep: d_pops[r * n_rows + i] in the caller's radius order; radii unsorted,
 *                                      equal, 0, +inf or NaN as for dc_hip_populations_dev; more than 8: ceil(n / 8)
 *                                      sweeps over the one image); rows outside [i_from, i_to): 0
 *   dc_hip_nearest_neighbors_fp32_dev  replaces density_clustering_cuda.cu:184-284; rows outside the range: "none" =
 *                                      (n_rows + 1, FLT_MAX)
 *   dc_hip_fp32_workspace_bytes        dc_hip_workspace_bytes for 1..32 columns, 0 outside them (and for no rows)
 *   dc_hip_fp32_plan                   how a call of that shape is run, decided on the host alone (no device needed):
 *                                      out[0] K-steps, out[1] floats per lane and tile of the image (a multiple of 4),
 *                                      out[2] query tiles per wave, population | neighbour << 16, out[3] radii per
 *                                      sweep | sweeps << 16, out[4] reference chunks, population | neighbour << 16,
 *                                      out[5] / out[6] dynamic LDS bytes per workgroup, population / neighbour,
 *                                      out[7] image bytes per 32-row tile | bytes the workspace keeps for it << 16.
 *                                      Query tiles, chunks and LDS are those of the call's FULL sweeps (radii per sweep
 *                                      radii each); the last sweep of a call whose count is no multiple of 8 holds
 *                                      fewer radii and is sized by the same rule: ask for that count to see it (one
 *                                      radius runs the one-radius kernel, which may take more query tiles per wave)
 * Flagged data (a non-finite or overflow-prone row, a NaN free energy) is answered by the direct kernels behind the
 * device-side gate.  The switches DC_MFMA32_CHUNKS / DC_MFMA32_WPB apply.
 * Refusals, all before a device is touched: n_cols outside 1..32, n_radii == 0, a NULL array or `out`, i_from > i_to or
 * i_to > n_rows: DC_ERR_INVALID_ARGUMENT; n_rows + 1 beyond uint32 or more than 65535 radii: DC_ERR_TOO_LARGE; a workspace smaller than
 * dc_hip_fp32_workspace_bytes, or none: DC_ERR_WORKSPACE.  n_rows == 0 or an empty range: DC_OK. */
DC_API size_t dc_hip_fp32_workspace_bytes(size_t n_rows, size_t n_cols, size_t n_radii);
DC_API int dc_hip_fp32_plan(size_t n_rows, size_t n_cols, size_t n_radii, uint32_t out[8]);
DC_API int dc_hip_populations_fp32_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* radii,
                                       size_t n_radii, size_t i_from, size_t i_to, uint32_t* d_pops, void* d_ws,
                                       size_t ws_bytes, void* stream);
DC_API int dc_hip_nearest_neighbors_fp32_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* d_fe,
                                             size_t i_from, size_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
                                             uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, size_t ws_bytes,
                                             void* stream);
/* ---- ... the PRUNED wide self population sweep (65..256 columns) -----------------------------------------------------------
 * dc_hip_populations_wide_dev's populations bit for bit, without the block pairs that cannot hold a pair within the
 * call's radii: the rows are put into a spatial order on columns 0 / 1 (cell keys, one stable sort), gathered into it,
 * every block of 128 positions gets a box in that plane, and a workgroup only runs the chains of the reference blocks
 * whose box lies within 1.0001 x the launch's largest r^2 of its query block's.  Entry points of their own; no
 * dc_variant value selects them.
 * d_pops: [n_radii][n_rows], fully overwritten.  Radii in any order, checked as dc_hip_populations_wide_dev checks them;
 * more than 8 radii run one launch per 8, each pruned by its own largest radius.
 * n_segments == 0: the whole sweep (`segment` is not read).  n_segments > 0: rank `segment` sweeps every n_segments-th query block (128
 * positions) of the order and writes the final counts of those rows, zeros elsewhere -- the sum over the segments is
 * the population (the contract of dc_hip_populations_segment_dev); a segment without a block gives zeros.  Flagged data
 * (a non-finite or overflow-prone row): the direct kernel answers behind the device-side gate, for a segment on the
 * row block dc_hip_populations_segment_dev uses.
 * Errors, all before a device is touched: segment >= n_segments > 0 and n_cols outside 65..256:
 * DC_ERR_INVALID_ARGUMENT; a workspace smaller than dc_hip_wide_pruned_workspace_bytes (or none): DC_ERR_WORKSPACE;
 * sizes: DC_ERR_TOO_LARGE as above; n_rows == 0 or n_radii == 0: DC_OK.
 * dc_hip_wide_pruned_workspace_bytes: 0 outside 65..256 columns (and for no rows), monotone in n_rows, never below
 * dc_hip_wide_workspace_bytes.  The workspace keeps the info head of the wide sweeps: dc_hip_wide_info_dev reads the
 * counters of the last pruned call; its tile pairs are the EVALUATED ones.
 * dc_hip_wide_pruned_order_dev: the order of the last pruned call in that workspace, position -> row, into d_perm
 * [n_rows] (block b of the order: positions 128 b .. 128 b + 127); a workspace that holds no order of that shape:
 * DC_ERR_INVALID_ARGUMENT.  Synchronises the stream. */
DC_API size_t dc_hip_wide_pruned_workspace_bytes(size_t n_rows, size_t n_cols, size_t n_radii);
DC_API int dc_hip_populations_wide_pruned_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* radii,
                                              size_t n_radii, size_t segment, size_t n_segments, uint32_t* d_pops,
                                              void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_wide_pruned_order_dev(const void* d_ws, size_t n_rows, size_t n_cols, uint32_t* d_perm, void* stream);
/* ---- ... the PRUNED wide self neighbour sweep (65..256 columns) ------------------------------------------------------------
 * dc_hip_nearest_neighbors_wide_dev's four outputs bit for bit -- indices, d2 bits, "none" = (n_rows + 1, FLT_MAX); ties
 * go to the lowest ROW -- in the spatial order and the workspace of dc_hip_populations_wide_pruned_dev
 * (dc_hip_wide_pruned_workspace_bytes(n_rows, n_cols, 1)), as the reference's CPU path and the sweeps below 65 columns
 * search outward and stop: a query block of 128 positions first meets the blocks next to it in the order, then the
 * blocks whose box lies within 1.0001 x the largest nn_d2 its rows have found, then those within 1.0001 x the largest
 * hd_d2 that hold a row of lower free energy than one of its own.  Entry point of its own; no dc_variant value selects it.
 * Outputs fully overwritten.  n_segments == 0: the whole sweep (`segment` is not read).  n_segments > 0: rank `segment`
 * sweeps every n_segments-th query block of the order, the partition dc_hip_populations_wide_pruned_dev uses; the rows
 * of other blocks hold "none", so partial results merge by the per-row minimum of (d2 bits << 32 | index) (the contract
 * of dc_hip_nearest_neighbors_segment_dev); a segment without a block gives "none" everywhere.  Flagged data (a
 * non-finite or overflow-prone row, a NaN free energy, as for dc_hip_nearest_neighbors_wide_dev): the direct kernel
 * answers behind the device-side gate, for a segment on the row block dc_hip_nearest_neighbors_segment_dev uses at these
 * widths; the counters read (0, 0, 0).  dc_hip_wide_info_dev reads the counters of the call (the EVALUATED tile pairs,
 * summed over its launches), dc_hip_wide_pruned_order_dev its order.
 * Errors, all before a device is touched: segment >= n_segments > 0 and n_cols outside 65..256:
 * DC_ERR_INVALID_ARGUMENT; a workspace smaller than dc_hip_wide_pruned_workspace_bytes (or none): DC_ERR_WORKSPACE;
 * sizes: DC_ERR_TOO_LARGE as above; n_rows == 0: DC_OK. */
DC_API int dc_hip_nearest_neighbors_wide_pruned_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* d_fe,
                                                    size_t segment, size_t n_segments, uint32_t* d_nn_idx, float* d_nn_d2,
                                                    uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, size_t ws_bytes,
                                                    void* stream);
/* ---- ... the neighbour blocks of a sharded run of it (the all-gather merge, 65..256 columns) ------------------------------
 * The contract of dc_hip_neighbors_block_*_dev in the order of the pruned wide sweep.  Rank g of G packs, right behind its
 * dc_hip_nearest_neighbors_wide_pruned_dev(segment g, G) and in the same workspace, the rows of the query blocks b = g
 * (mod G) of the order, 128 positions each, by local position into d_block [4][block_rows] uint32: nn_idx, nn_d2 bits,
 * hd_idx, hd_d2 bits; pad entries hold "none" = (n_rows + 1, FLT_MAX).  block_rows =
 * dc_hip_neighbors_block_rows_wide(n_rows, n_cols, G): the larger of the largest segment in positions and the largest
 * row block of the reference's partition (n_rows / G rows, the last rank takes the remainder), plus 32.  The last 32
 * entries of plane 0 are the layout header: mark | by-position flag, positions, block size 128, segment count, deal,
 * and a 64-bit hash of the order (words 0..6; the rest 0).  Flagged data, which the sweep answered from the direct
 * kernel on the reference's row block: row blocks -- pack and unpack decide on the device from the word the sweep's gate
 * left in the workspace, without a host synchronisation.
 * The unpack takes d_blocks [G][4][block_rows], the blocks of all ranks in rank order, in a workspace that holds the
 * same order (every rank of a run derives it from the same rows), and writes the four arrays by row.  Its kernel first
 * compares the G headers with the layout of its own workspace: on a mismatch it writes NOTHING and records the verdict in
 * the workspace, where dc_hip_wide_layout_status_dev reads it (*mismatch = 1; synchronises the stream); the verdict is
 * that of the last unpack, a clean one reads 0.
 * Errors, all before a device is touched: segment >= n_segments, n_segments == 0 and n_cols outside 65..256:
 * DC_ERR_INVALID_ARGUMENT; a workspace smaller than dc_hip_wide_pruned_workspace_bytes(n_rows, n_cols, 1) (or none):
 * DC_ERR_WORKSPACE; sizes: DC_ERR_TOO_LARGE as above; n_rows == 0: DC_OK.  dc_hip_neighbors_block_rows_wide is 0 outside
 * 65..256 columns, for no rows and for no segments. */
DC_API size_t dc_hip_neighbors_block_rows_wide(size_t n_rows, size_t n_cols, size_t n_segments);
DC_API int dc_hip_neighbors_block_pack_wide_dev(const uint32_t* d_nn_idx, const float* d_nn_d2, const uint32_t* d_hd_idx,
                                                const float* d_hd_d2, size_t n_rows, size_t n_cols, size_t segment,
                                                size_t n_segments, void* d_ws, size_t ws_bytes, uint32_t* d_block,
                                                void* stream);
DC_API int dc_hip_neighbors_block_unpack_wide_dev(const uint32_t* d_blocks, size_t n_rows, size_t n_cols, size_t n_segments,
                                                  void* d_ws, size_t ws_bytes, uint32_t* d_nn_idx, float* d_nn_d2,
                                                  uint32_t* d_hd_idx, float* d_hd_d2, void* stream);
DC_API int dc_hip_wide_layout_status_dev(const void* d_ws, int* mismatch, void* stream);
/* ---- ... and the same blocks at 257..1024 columns ---------------------------------------------------------------------------
 * The four calls above behind dc_hip_nearest_neighbors_xwide_pruned_dev(segment g, G), in its workspace
 * (dc_hip_xwide_pruned_workspace_bytes(n_rows, n_cols, 1)): the same bodies and kernels in the layout of these widths.  Each
 * takes the argument list of its _wide namesake, keeps its contract -- blocks by local position; row blocks on flagged
 * data, chosen on the device from the word the sweep's gate read; the layout header with the hash of the order; an unpack
 * that compares all G headers with the header of its own workspace before it writes anything; a workspace that holds no
 * signed order of this shape packs under a mark no unpack accepts; rows read from the order are checked against n_rows
 * -- and refuses in the same order with the same codes, before a device is touched, naming itself.  n_cols outside
 * 257..1024: DC_ERR_INVALID_ARGUMENT; dc_hip_neighbors_block_rows_xwide is 0 there (the same number as
 * dc_hip_neighbors_block_rows_wide otherwise: a block is no function of the width).  The header does not carry the width:
 * what an unpack holds a block to is the layout -- shape, deal and the hash of the order -- so a block packed at another
 * width is refused through the order it was packed by. */
DC_API size_t dc_hip_neighbors_block_rows_xwide(size_t n_rows, size_t n_cols, size_t n_segments);
DC_API int dc_hip_neighbors_block_pack_xwide_dev(const uint32_t* d_nn_idx, const float* d_nn_d2, const uint32_t* d_hd_idx,
                                                 const float* d_hd_d2, size_t n_rows, size_t n_cols, size_t segment,
                                                 size_t n_segments, void* d_ws, size_t ws_bytes, uint32_t* d_block,
                                                 void* stream);
DC_API int dc_hip_neighbors_block_unpack_xwide_dev(const uint32_t* d_blocks, size_t n_rows, size_t n_cols, size_t n_segments,
                                                   void* d_ws, size_t ws_bytes, uint32_t* d_nn_idx, float* d_nn_d2,
                                                   uint32_t* d_hd_idx, float* d_hd_d2, void* stream);
DC_API int dc_hip_xwide_layout_status_dev(const void* d_ws, int* mismatch, void* stream);
/* ---- ... and their cross form: query frames against a reference trajectory at 65..256 columns ------------------------
 * The wide sweep over a rectangle Q x R: the contract of the "cross sweeps" block above -- populations without a self
 * term, nn[q] the lexicographic minimum of (d2, j) over ALL j with no exclusion, nn_hd[q] the same over
 * { j : fe_ref[j] < fe_query[q] } compared as IEEE, d_fe_query == NULL: nn only (d_fe_ref, d_hd_idx, d_hd_d2 may be
 * NULL and are not written), "none" = (n_ref + 1, FLT_MAX), 0 / "none" outside [i_from, i_to), outputs fully
 * overwritten, d_query == d_ref allowed, radii in any order -- with results bit-identical to dc_hip_*_cross_dev under
 * DC_VARIANT_DIRECT.  One origin and one scale serve Q and R together; one matrix-core chain per tile pair serves up
 * to 8 radii, more radii run one launch per 8.  Entry points of their own: no dc_variant value selects them, and
 * dc_hip_*_cross_dev keep sending rows wider than 64 columns to the direct kernels.
 * Flagged data -- a non-finite or overflow-prone row in Q or in R -- is answered by the direct kernels behind the
 * device-side gate, without a host synchronisation.  A NaN in fe_query or fe_ref does NOT flag the data: the sweep has
 * no order by free energy, its test is the same IEEE comparison as the direct kernel's (a NaN is never lower and has no
 * lower neighbour), so the matrix-core kernel answers such a call too.
 * n_cols outside 65..256: DC_ERR_INVALID_ARGUMENT; a workspace smaller than dc_hip_cross_wide_workspace_bytes:
 * DC_ERR_WORKSPACE; n_ref + 1 and n_query must fit uint32: DC_ERR_TOO_LARGE; n_query == 0, n_ref == 0 or an empty
 * range: DC_OK with zeros / "none".
 * dc_hip_cross_wide_workspace_bytes: 0 outside 65..256 columns and for an empty side (such a call takes d_ws == NULL; a
 * workspace that is given anyway reports that nothing was swept), monotone in either row count.  The workspace keeps the
 * info head of the wide self sweeps: dc_hip_wide_info_dev reads the counters of the last cross-wide call in it. */
DC_API size_t dc_hip_cross_wide_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols, size_t n_radii);
DC_API int dc_hip_populations_cross_wide_dev(const float* d_query, size_t n_query, const float* d_ref, size_t n_ref,
                                             size_t n_cols, const float* radii, size_t n_radii, size_t i_from,
                                             size_t i_to, uint32_t* d_pops, void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_nearest_neighbors_cross_wide_dev(const float* d_query, size_t n_query, const float* d_ref,
                                                   size_t n_ref, size_t n_cols, const float* d_fe_query,
                                                   const float* d_fe_ref, size_t i_from, size_t i_to,
                                                   uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                                   float* d_hd_d2, void* d_ws, size_t ws_bytes, void* stream);
/* ---- ... and the same sweeps for rows of 257..1024 columns ("extra-wide") ---------------------------------------------------
 * The unpruned self and cross sweeps above at 257..1024 columns: the same kernels (their chain streams along K and takes
 * its length at run time), the same contracts, results bit-identical to DC_VARIANT_DIRECT -- beyond 400 columns that is
 * the column-chunked direct kernel, which also answers flagged data behind the device-side gate.  Every entry point takes
 * the argument list of its _wide_ namesake and refuses in the same order, naming itself; n_cols outside 257..1024:
 * DC_ERR_INVALID_ARGUMENT.  The workspace has a layout of its own (column sums and means for 1024 columns behind the
 * header, the operand images from byte 13 312 on; about 6 KB per row and image at 1024 columns), so a workspace of one
 * family never serves the other: dc_hip_xwide_workspace_bytes / dc_hip_cross_xwide_workspace_bytes are 0 outside
 * 257..1024 columns, for no rows and for an empty side, and monotone in the row counts.  The info head is that of the
 * wide sweeps: dc_hip_wide_info_dev reads the counters of the last call.  The pruned self sweeps follow below, the
 * pruned cross sweeps behind those of 65..256 columns; no session and no resident reference exists at these widths; no
 * dc_variant value selects them. */
DC_API size_t dc_hip_xwide_workspace_bytes(size_t n_rows, size_t n_cols, size_t n_radii);
DC_API int dc_hip_populations_xwide_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* radii,
                                        size_t n_radii, size_t i_from, size_t i_to, uint32_t* d_pops, void* d_ws,
                                        size_t ws_bytes, void* stream);
DC_API int dc_hip_nearest_neighbors_xwide_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* d_fe,
                                              size_t i_from, size_t i_to, uint32_t* d_nn_idx, float* d_nn_d2,
                                              uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, size_t ws_bytes,
                                              void* stream);
DC_API size_t dc_hip_cross_xwide_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols, size_t n_radii);
DC_API int dc_hip_populations_cross_xwide_dev(const float* d_query, size_t n_query, const float* d_ref, size_t n_ref,
                                              size_t n_cols, const float* radii, size_t n_radii, size_t i_from,
                                              size_t i_to, uint32_t* d_pops, void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_nearest_neighbors_cross_xwide_dev(const float* d_query, size_t n_query, const float* d_ref,
                                                    size_t n_ref, size_t n_cols, const float* d_fe_query,
                                                    const float* d_fe_ref, size_t i_from, size_t i_to,
                                                    uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                                    float* d_hd_d2, void* d_ws, size_t ws_bytes, void* stream);
/* ---- ... and the PRUNED self population and neighbour sweeps at 257..1024 columns ------------------------------------------
 * dc_hip_populations_wide_pruned_dev and dc_hip_nearest_neighbors_wide_pruned_dev at 257..1024 columns: the spatial order
 * on columns 0 / 1, the block boxes, the segments (every n_segments-th query block of the order; n_segments == 0: the
 * whole sweep, `segment` is not read) and the three launches of the neighbour sweep are theirs, the pruning rules take
 * the floors of these widths.  Results are bit-identical to dc_hip_populations_xwide_dev /
 * dc_hip_nearest_neighbors_xwide_dev and to DC_VARIANT_DIRECT.  Each entry point takes the argument list of its
 * _wide_pruned_ namesake and refuses in the same order, before a device is touched, naming itself; n_cols outside
 * 257..1024: DC_ERR_INVALID_ARGUMENT; a workspace smaller than dc_hip_xwide_pruned_workspace_bytes (or none):
 * DC_ERR_WORKSPACE.  dc_hip_xwide_pruned_workspace_bytes: 0 outside 257..1024 columns and for no rows, monotone in
 * n_rows, never below dc_hip_xwide_workspace_bytes (the head is that layout); dc_hip_wide_pruned_workspace_bytes stays 0
 * at these widths and the _wide_pruned_ entry points refuse them.  Flagged data and NaN free energies: the gated direct
 * kernel answers (beyond 400 columns the column-chunked one), a segment call the row block of
 * dc_hip_populations_segment_dev / dc_hip_nearest_neighbors_segment_dev, no host synchronisation.  dc_hip_wide_info_dev
 * reads the counters of the last call (EVALUATED tile pairs), dc_hip_xwide_pruned_order_dev its order. */
DC_API size_t dc_hip_xwide_pruned_workspace_bytes(size_t n_rows, size_t n_cols, size_t n_radii);
DC_API int dc_hip_populations_xwide_pruned_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* radii,
                                               size_t n_radii, size_t segment, size_t n_segments, uint32_t* d_pops,
                                               void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_nearest_neighbors_xwide_pruned_dev(const float* d_coords, size_t n_rows, size_t n_cols, const float* d_fe,
                                                     size_t segment, size_t n_segments, uint32_t* d_nn_idx, float* d_nn_d2,
                                                     uint32_t* d_hd_idx, float* d_hd_d2, void* d_ws, size_t ws_bytes,
                                                     void* stream);
DC_API int dc_hip_xwide_pruned_order_dev(const void* d_ws, size_t n_rows, size_t n_cols, uint32_t* d_perm, void* stream);
/* ---- ... the PRUNED wide cross population sweep (65..256 columns) ----------------------------------------------------------
 * dc_hip_populations_cross_wide_dev's populations bit for bit, without the block pairs that cannot hold a pair within
 * the call's radii.  Statistics, origin and scale are those of the cross form.  ONE cell grid on columns 0 / 1 covers the
 * queries [i_from, i_to) and the reference together (its cell sized by the reference's row count); the reference and the
 * query range are each sorted by its keys, gathered and boxed per block of 128 positions, and a workgroup only runs the
 * chains of the reference blocks whose box lies within 1.0001 x the launch's largest r^2 of its query block's.  Entry
 * points of their own; no dc_variant value selects them.
 * Arguments, refusals and contract are those of dc_hip_populations_cross_wide_dev: no self term; d_pops [n_radii][n_query]
 * fully overwritten, zeros outside [i_from, i_to); radii in any order, more than 8 run one launch per 8, each pruned by
 * its own largest radius; d_query == d_ref allowed; n_query == 0, n_ref == 0 or an empty range: DC_OK with zeros.
 * Flagged data -- a non-finite or overflow-prone row in Q or in R -- is answered by the direct kernel behind the
 * device-side gate, without a host synchronisation; the counters then read (0, 0, 0).
 * n_cols outside 65..256: DC_ERR_INVALID_ARGUMENT; a workspace smaller than dc_hip_cross_wide_pruned_workspace_bytes:
 * DC_ERR_WORKSPACE; n_ref + 1 and n_query must fit uint32: DC_ERR_TOO_LARGE -- all before a device is touched.
 * dc_hip_cross_wide_pruned_workspace_bytes: 0 outside 65..256 columns and for an empty side, monotone in either row
 * count, never below dc_hip_cross_wide_workspace_bytes.  The workspace keeps the info head of the wide sweeps:
 * dc_hip_wide_info_dev reads the counters of the last call; its tile pairs are the EVALUATED ones.
 * dc_hip_cross_wide_pruned_order_dev: both orders of the last call in that workspace, position -> row: d_perm_q
 * [n_query_range = i_to - i_from] names rows of Q (query block b: positions 128 b .. 128 b + 127), d_perm_r [n_ref] rows
 * of R.  A workspace that holds no cross order of that shape -- a self order included -- : DC_ERR_INVALID_ARGUMENT.
 * Synchronises the stream. */
DC_API size_t dc_hip_cross_wide_pruned_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols, size_t n_radii);
DC_API int dc_hip_populations_cross_wide_pruned_dev(const float* d_query, size_t n_query, const float* d_ref, size_t n_ref,
                                                    size_t n_cols, const float* radii, size_t n_radii, size_t i_from,
                                                    size_t i_to, uint32_t* d_pops, void* d_ws, size_t ws_bytes,
                                                    void* stream);
DC_API int dc_hip_cross_wide_pruned_order_dev(const void* d_ws, size_t n_query_range, size_t n_ref, size_t n_cols,
                                              uint32_t* d_perm_q, uint32_t* d_perm_r, void* stream);
/* ---- ... and the PRUNED wide cross neighbour sweep (65..256 columns) --------------------------------------------------------
 * dc_hip_nearest_neighbors_cross_wide_dev's four outputs bit for bit -- indices, d2 bits, "none" -- in the two orders and
 * the workspace of dc_hip_populations_cross_wide_pruned_dev (dc_hip_cross_wide_pruned_workspace_bytes(n_query, n_ref,
 * n_cols, 1)).  The call prepares both orders itself and trusts none left by an earlier call.  A query block of 128
 * positions first meets ONE reference block, the one with a live row whose box centre is nearest to its own box centre in
 * the (column 0, column 1) plane (the lowest block on a tie), then the blocks whose box lies within 1.0001 x the largest
 * nn_d2 its rows have found, then those within 1.0001 x the largest hd_d2 that hold a row of lower free energy than one
 * of its own.  Entry point of its own; no dc_variant value selects it.
 * Arguments, refusals and contract are those of dc_hip_nearest_neighbors_cross_wide_dev: nn[q] the least (d2, ROW of R)
 * over all j with no exclusion; nn_hd[q] the same over { j : fe_ref[j] < fe_query[q] }, compared as IEEE;
 * d_fe_query == NULL: nn only (d_fe_ref, d_hd_idx, d_hd_d2 may be NULL and are not written, two launches instead of
 * three); "none" = (n_ref + 1, FLT_MAX), also outside [i_from, i_to); outputs fully overwritten; d_query == d_ref
 * allowed; n_query == 0, n_ref == 0 or an empty range: DC_OK with "none".
 * Flagged data -- a non-finite or overflow-prone row in Q or in R, OR a NaN in fe_query[i_from, i_to) or fe_ref (the third
 * launch rests on the least and largest free energy per block) -- is answered by the direct kernel behind the
 * device-side gate, without a host synchronisation: the same IEEE comparison, so the results still equal the unpruned
 * call's; the counters then read (0, 0, 0).
 * n_cols outside 65..256: DC_ERR_INVALID_ARGUMENT; a workspace smaller than dc_hip_cross_wide_pruned_workspace_bytes (or
 * none): DC_ERR_WORKSPACE; n_ref + 1 and n_query must fit uint32: DC_ERR_TOO_LARGE -- all before a device is touched.
 * dc_hip_wide_info_dev reads the counters of the call (the EVALUATED tile pairs, summed over its launches; no block pair
 * is counted twice), dc_hip_cross_wide_pruned_order_dev its two orders. */
DC_API int dc_hip_nearest_neighbors_cross_wide_pruned_dev(const float* d_query, size_t n_query, const float* d_ref,
                                                          size_t n_ref, size_t n_cols, const float* d_fe_query,
                                                          const float* d_fe_ref, size_t i_from, size_t i_to,
                                                          uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                                          float* d_hd_d2, void* d_ws, size_t ws_bytes, void* stream);
/* ---- ... and both PRUNED wide cross sweeps at 257..1024 columns ------------------------------------------------------------
 * dc_hip_populations_cross_wide_pruned_dev and dc_hip_nearest_neighbors_cross_wide_pruned_dev at 257..1024 columns: the
 * one cell grid on columns 0 / 1, the two orders, the block boxes, the seed block and the three launches of the neighbour
 * sweep are theirs; the pruning rules take the floors of these widths (a positive radius below 2^-61 prunes as 2^-61
 * does) and the later launches of the neighbour sweep start from bounds formed with the factor of these widths.  Results
 * are bit-identical to dc_hip_populations_cross_xwide_dev / dc_hip_nearest_neighbors_cross_xwide_dev and to
 * DC_VARIANT_DIRECT.  Each entry point takes the argument list of its _cross_wide_pruned_ namesake and refuses in the same
 * order, before a device is touched, naming itself; n_cols outside 257..1024: DC_ERR_INVALID_ARGUMENT; a workspace
 * smaller than dc_hip_cross_xwide_pruned_workspace_bytes (or none): DC_ERR_WORKSPACE.
 * dc_hip_cross_xwide_pruned_workspace_bytes: 0 outside 257..1024 columns and for an empty side, monotone in either row
 * count, never below dc_hip_cross_xwide_workspace_bytes (the head is that layout); a workspace of one family never serves
 * the other: dc_hip_cross_wide_pruned_workspace_bytes stays 0 at these widths and the _cross_wide_pruned_ entry points
 * refuse them.  Flagged data -- a non-finite or overflow-prone row in Q or in R, a NaN free energy -- is answered by the
 * gated direct kernel (beyond 400 columns the column-chunked one), no host synchronisation; the counters then read
 * (0, 0, 0).  dc_hip_wide_info_dev reads the counters of the last call (EVALUATED tile pairs),
 * dc_hip_cross_xwide_pruned_order_dev its two orders (a self order or an order of the 65..256 family is refused).  No
 * dc_variant value selects them; the resident reference dc_reference_xwide below runs them, and through it the assigner's
 * path 3. */
DC_API size_t dc_hip_cross_xwide_pruned_workspace_bytes(size_t n_query, size_t n_ref, size_t n_cols, size_t n_radii);
DC_API int dc_hip_populations_cross_xwide_pruned_dev(const float* d_query, size_t n_query, const float* d_ref, size_t n_ref,
                                                     size_t n_cols, const float* radii, size_t n_radii, size_t i_from,
                                                     size_t i_to, uint32_t* d_pops, void* d_ws, size_t ws_bytes,
                                                     void* stream);
DC_API int dc_hip_nearest_neighbors_cross_xwide_pruned_dev(const float* d_query, size_t n_query, const float* d_ref,
                                                           size_t n_ref, size_t n_cols, const float* d_fe_query,
                                                           const float* d_fe_ref, size_t i_from, size_t i_to,
                                                           uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                                           float* d_hd_d2, void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_cross_xwide_pruned_order_dev(const void* d_ws, size_t n_query_range, size_t n_ref, size_t n_cols,
                                               uint32_t* d_perm_q, uint32_t* d_perm_r, void* stream);

/* ---- ... and a RESIDENT REFERENCE for the two (65..256 columns) -------------------------------------------------------------
 * The two pruned wide cross sweeps for a caller who streams batches of queries against ONE reference: the reference is
 * prepared once, when it is opened -- origin, scale, grid, its order, its gathered rows, boxes, operand image and norms --,
 * and a batch pays for itself alone.  The statistics cannot depend on a batch: the origin is the column mean of the
 * reference, the grid its extent in columns 0 / 1 (a query outside it lands in an edge cell; its block's box is still
 * formed from its own floats), and the scale is that of FOUR TIMES the reference's largest |x - mean|^2: a query up to
 * twice as far from the origin as the farthest reference frame runs on the matrix cores.
 * The handle is a small host object.  It BORROWS d_ref and d_ws until it is closed, and d_query from
 * dc_hip_reference_wide_stage_dev until the last sweep of that batch: all must stay valid and unchanged for that long.
 * d_fe_ref and d_fe_query are read by the call they are given to and not kept.  Calls on one handle are ordered by the
 * caller: on one stream, or with synchronisation between them.  Nothing here synchronises with the host but the two readers.
 *   workspace_bytes  a region sized by (n_ref, n_cols) that stays, one sized by (max_batch, n_cols) that a batch
 *                    rewrites, and the sort's scratch; 0 outside 65..256 columns or for a zero count; monotone in each argument
 *   open             prepares the reference (once per handle: `reference_preparations` of the info call counts the runs)
 *   set_free_energies  fe_ref[n_ref], as dc_hip_nearest_neighbors_cross_wide_dev takes it; may be called again with new values
 *   stage            the batch: ONE pass over its rows (the gate, and the cell keys), its order, gathered rows, boxes and
 *                    operand image.  n_query <= max_batch; n_query == 0 stages an empty batch, whose sweeps return DC_OK
 *                    and write nothing
 *   populations      d_pops[n_radii][n_query] = dc_hip_populations_cross_wide_dev's over the whole batch, bit for bit: no
 *                    self term, radii (host pointer) in any order, one launch per 8, each pruned by its own largest radius
 *   nearest          the four arrays of dc_hip_nearest_neighbors_cross_wide_dev over the whole batch, bit for bit: the least
 *                    (d2, ROW of R); "none" = (n_ref + 1, FLT_MAX); d_fe_query == NULL: nn only, the hd outputs may be NULL
 *                    and are not written
 * The two sweeps of a staged batch run in either order and any number of times without a second preparation.
 * Flagged data is answered by the direct kernels behind the device-side gate, without a host synchronisation, with the
 * same results; the counters then read (0, 0, 0).  `answered` of the info call says who answered the LAST sweep:
 *   0 the matrix cores;  1 the direct kernels, the reference holds a non-finite or overflow-prone row;  2 the direct
 *   kernels, the staged batch holds a row that is non-finite or farther from the origin than the scale allows;  3 the
 *   direct kernel, a NaN in fe_ref or in d_fe_query (the neighbour sweep with free energies only: populations, and
 *   neighbours without free energies, stay on the matrix cores).
 * A flag lasts as long as what raised it: the batch's until the next stage, the free energies' until they are set again.
 * info (tiles, mfmas, exact_pairs as dc_hip_wide_info_dev gives them, of the last sweep; any pointer may be NULL) and
 * order (d_perm_q[n_query of the staged batch], d_perm_r[n_ref], position -> row; either may be NULL) SYNCHRONISE.
 * Refusals, all before a device is touched, dc_hip_last_error names the function: n_cols outside 65..256, n_ref == 0,
 * max_batch == 0, a NULL array, handle or `out`, n_query > max_batch, a sweep before any stage, d_fe_query before free
 * energies were set: DC_ERR_INVALID_ARGUMENT; n_ref + 1 or max_batch beyond uint32, or either count times n_cols beyond
 * the element arithmetic (as the cross calls check them): DC_ERR_TOO_LARGE; a workspace smaller than
 * dc_hip_reference_wide_workspace_bytes, or none: DC_ERR_WORKSPACE.  On a refusal of open *out is NULL. */
typedef struct dc_reference_wide dc_reference_wide;
DC_API size_t dc_hip_reference_wide_workspace_bytes(size_t n_ref, size_t n_cols, size_t max_batch);
DC_API int dc_hip_reference_wide_open_dev(const float* d_ref, size_t n_ref, size_t n_cols, size_t max_batch, void* d_ws,
                                          size_t ws_bytes, void* stream, dc_reference_wide** out);
DC_API void dc_hip_reference_wide_close(dc_reference_wide* reference);
DC_API int dc_hip_reference_wide_set_free_energies_dev(dc_reference_wide* reference, const float* d_fe_ref, void* stream);
DC_API int dc_hip_reference_wide_stage_dev(dc_reference_wide* reference, const float* d_query, size_t n_query, void* stream);
DC_API int dc_hip_reference_wide_populations_dev(dc_reference_wide* reference, const float* radii, size_t n_radii,
                                                 uint32_t* d_pops, void* stream);
DC_API int dc_hip_reference_wide_nearest_dev(dc_reference_wide* reference, const float* d_fe_query, uint32_t* d_nn_idx,
                                             float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* stream);
DC_API int dc_hip_reference_wide_info_dev(dc_reference_wide* reference, uint64_t* tiles, uint64_t* mfmas,
                                          uint64_t* exact_pairs, uint32_t* answered, uint32_t* reference_preparations,
                                          void* stream);
DC_API int dc_hip_reference_wide_order_dev(dc_reference_wide* reference, uint32_t* d_perm_q, uint32_t* d_perm_r, void* stream);

/* ---- ... and a RESIDENT REFERENCE for rows of 257..1024 columns ----------------------------------------------------------------
 * dc_reference_wide for the two pruned cross sweeps of 257..1024 columns (dc_hip_*_cross_xwide_pruned_dev): the same
 * resident form -- origin, grid and scale from the reference alone, the scale that of FOUR TIMES its largest
 * |x - mean|^2, one gate pass per batch -- in the workspace layout of these widths.  Each entry point takes the argument
 * list of its _wide_ namesake, keeps its contract and refuses in the same order, before a device is touched, naming
 * itself; n_cols outside 257..1024: DC_ERR_INVALID_ARGUMENT.  Results are those of dc_hip_populations_cross_xwide_dev /
 * dc_hip_nearest_neighbors_cross_xwide_dev and of DC_VARIANT_DIRECT, bit for bit.
 * dc_hip_reference_xwide_workspace_bytes: 0 outside 257..1024 columns or for a zero count, monotone in each argument; a
 * workspace of one kind never serves the other (dc_hip_reference_wide_workspace_bytes stays 0 at these widths).
 * Flagged data -- `answered` 1..3 as above -- is answered by the gated direct kernels (beyond 400 columns the
 * column-chunked ones), no host synchronisation.
 * The band is formed from 4 M_ref where a per-call sweep forms it from the batch's and the reference's own extent: more
 * pairs take the exact path (each a canonical sum of n_cols terms).  Measured on dense data (20 000 x 100 000 x 512,
 * 2 000 x 100 000 x 512, 10 000 x 50 000 x 1024, one MI355X): stage + populations takes 0.46, 0.73 and 0.45 x the speed of
 * one dc_hip_populations_cross_xwide_pruned_dev call (3.9 x the exact pairs), stage + populations + nearest 0.57, 0.99 and
 * 0.52 x.  For ONE batch per reference, or for the least time per population call, use the per-call entry points above.  The
 * handle pays where the reference's own work repeats: a whole assignment of a batch (reference self sweep included on the
 * other side) is 1.9 - 10.9 x faster on it, the host assigner's path 3 3.2 - 9.8 x faster than path 2. */
typedef struct dc_reference_xwide dc_reference_xwide;
DC_API size_t dc_hip_reference_xwide_workspace_bytes(size_t n_ref, size_t n_cols, size_t max_batch);
DC_API int dc_hip_reference_xwide_open_dev(const float* d_ref, size_t n_ref, size_t n_cols, size_t max_batch, void* d_ws,
                                           size_t ws_bytes, void* stream, dc_reference_xwide** out);
DC_API void dc_hip_reference_xwide_close(dc_reference_xwide* reference);
DC_API int dc_hip_reference_xwide_set_free_energies_dev(dc_reference_xwide* reference, const float* d_fe_ref, void* stream);
DC_API int dc_hip_reference_xwide_stage_dev(dc_reference_xwide* reference, const float* d_query, size_t n_query, void* stream);
DC_API int dc_hip_reference_xwide_populations_dev(dc_reference_xwide* reference, const float* radii, size_t n_radii,
                                                  uint32_t* d_pops, void* stream);
DC_API int dc_hip_reference_xwide_nearest_dev(dc_reference_xwide* reference, const float* d_fe_query, uint32_t* d_nn_idx,
                                              float* d_nn_d2, uint32_t* d_hd_idx, float* d_hd_d2, void* stream);
DC_API int dc_hip_reference_xwide_info_dev(dc_reference_xwide* reference, uint64_t* tiles, uint64_t* mfmas,
                                           uint64_t* exact_pairs, uint32_t* answered, uint32_t* reference_preparations,
                                           void* stream);
DC_API int dc_hip_reference_xwide_order_dev(dc_reference_xwide* reference, uint32_t* d_perm_q, uint32_t* d_perm_r, void* stream);

/* ---- ... and the radius graph on the wide self sweep (65..256 columns) --------------------------------------------------
 * The one-radius population sweep with a sink on its two decision points, the accumulator window and the exact drain.
 * Entry points of their own, like the sweeps above: no dc_variant value selects them, and dc_hip_radius_pairs_dev,
 * dc_hip_radius_min_edge[_segment]_dev, dc_hip_radius_forest and the sessions keep sending rows wider than 64 columns
 * to the direct kernels.  Workspace: dc_hip_wide_workspace_bytes(n_rows, n_cols, 1); dc_hip_wide_info_dev reads the
 * counters of the last graph call in it.  n_cols outside 65..256: DC_ERR_INVALID_ARGUMENT; a short or NULL workspace:
 * DC_ERR_WORKSPACE; sizes as for the calls they mirror (the min-edge row limit included); n_rows == 0: DC_OK -- all
 * checked before a device is touched.  Flagged data (a non-finite or overflow-prone row): the direct kernels answer
 * behind the device-side gate, without a host synchronisation, counters (0, 0, 0).
 *
 * dc_hip_radius_pairs_wide_dev: the contract of dc_hip_radius_pairs_dev -- every unordered pair {i, j}, i != j, with
 * canonical d2 < r2 exactly once, in no particular order; d_pops fully overwritten (1 + number of partners); d_pairs
 * NULL with capacity 0 counts only; *d_count is the full count even when it exceeds capacity, in which case exactly
 * `capacity` distinct valid pairs are written and nothing beyond; a NaN, 0 or negative r2 holds no pair. */
DC_API int dc_hip_radius_pairs_wide_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2, uint32_t* d_pops,
                                        uint32_t* d_pairs, size_t capacity, unsigned long long* d_count, void* d_ws,
                                        size_t ws_bytes, void* stream);
/* the contract of dc_hip_radius_min_edge_segment_dev; n_segments == 0: the whole round.  A segment is the reference's
 * row block (density_clustering_cuda.cu:149,165-169), the partition that call uses at these widths, so the outputs of
 * a segment are array-equal to its outputs: d_best merges by unsigned minimum, d_pops by summation.  Both outputs are
 * preset by the call (~0 / 0). */
DC_API int dc_hip_radius_min_edge_wide_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                           const uint32_t* d_comp, const uint32_t* d_rank, size_t segment,
                                           size_t n_segments, unsigned long long* d_best, uint32_t* d_pops, void* d_ws,
                                           size_t ws_bytes, void* stream);
/* host-pointer form with the contract of dc_hip_radius_forest (rank, edges, n_edges, n_rounds as there), on ONE device
 * and without a session: one upload, then Boruvka rounds of dc_hip_radius_min_edge_wide_dev in one workspace with the
 * components merged on the host.  A rank that is no permutation: DC_ERR_INVALID_ARGUMENT before a device is touched. */
DC_API int dc_hip_radius_forest_wide(const float* coords, size_t n_rows, size_t n_cols, float r2, const uint32_t* rank,
                                     int device, uint32_t* edges, size_t* n_edges, uint32_t* n_rounds);

/* ---- ... and the PRUNED radius graph (65..256 columns) -------------------------------------------------------------------
 * The three calls above on the pruned wide sweep: the rows in the spatial order of dc_hip_populations_wide_pruned_dev, a
 * box per block of 128 positions, and only the chains of the reference blocks whose box lies within 1.0001 x r2 of the
 * query block's.  The same results; entry points of their own, no dc_variant value selects them.  Workspace:
 * dc_hip_wide_pruned_workspace_bytes(n_rows, n_cols, 1); dc_hip_wide_info_dev reads the counters of the last call in it
 * (the EVALUATED tile pairs) and dc_hip_wide_pruned_order_dev its order.  Refusals as for the calls they mirror, with the
 * same codes, all before a device is touched.  Flagged data: the direct kernels answer on the original rows behind the
 * device-side gate, a segment on the reference's row block, counters (0, 0, 0), no host synchronisation.
 *
 * dc_hip_radius_pairs_wide_pruned_dev: arguments and contract of dc_hip_radius_pairs_wide_dev.  Every unordered pair once,
 * in no particular order, and in NO ORDER WITHIN A PAIR: (i, j) may come with i > j (the sweep decides which of the two
 * meetings of a pair emits on positions of the order and writes the rows behind them).
 * dc_hip_radius_min_edge_wide_pruned_dev: arguments of dc_hip_radius_min_edge_wide_dev.  n_segments == 0: the whole
 * round (`segment` is not read), outputs array-equal to that call's.  n_segments > 0: rank `segment` takes every
 * n_segments-th query block of the order, the partition dc_hip_populations_wide_pruned_dev uses; d_best merges by
 * unsigned minimum, d_pops (final for the rows of its blocks, 0 elsewhere) by summation.  Both outputs are preset by the
 * call.  The same row limit.
 * dc_hip_radius_forest_wide_pruned: the host-pointer contract of dc_hip_radius_forest_wide; the order is built once per
 * forest. */
DC_API int dc_hip_radius_pairs_wide_pruned_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                               uint32_t* d_pops, uint32_t* d_pairs, size_t capacity,
                                               unsigned long long* d_count, void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_radius_min_edge_wide_pruned_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                                  const uint32_t* d_comp, const uint32_t* d_rank, size_t segment,
                                                  size_t n_segments, unsigned long long* d_best, uint32_t* d_pops,
                                                  void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_radius_forest_wide_pruned(const float* coords, size_t n_rows, size_t n_cols, float r2,
                                            const uint32_t* rank, int device, uint32_t* edges, size_t* n_edges,
                                            uint32_t* n_rounds);

/* ---- ... and the radius graph at 257..1024 columns, unpruned and pruned ---------------------------------------------------
 * The six calls above in the layouts of these widths: the same bodies, the same two kernel instances over a chain of up
 * to 193 MFMAs.  Each takes the argument list of its _wide_ / _wide_pruned_ namesake, keeps its contract -- every
 * unordered pair with canonical d2 < r2 exactly once (the pruned form: in no order within a pair); *d_count exact beyond
 * the capacity and exactly `capacity` distinct valid pairs written; a NaN, 0 or negative r2 holds no pair; both min-edge
 * outputs preset by the call; an unpruned min-edge segment is the reference's row block, a pruned one every
 * n_segments-th query block of the order (d_best merges by unsigned minimum, d_pops by summation); the order is built
 * once per forest; the same min-edge row limit -- and refuses in the same order with the same codes, before a device is
 * touched, naming itself.  n_cols outside 257..1024: DC_ERR_INVALID_ARGUMENT.
 * Workspace: dc_hip_xwide_workspace_bytes(n_rows, n_cols, 1) for the unpruned calls,
 * dc_hip_xwide_pruned_workspace_bytes(n_rows, n_cols, 1) for the pruned ones; a workspace of one family never serves the
 * other.  dc_hip_wide_info_dev reads the counters of the last call (the pruned calls: the EVALUATED tile pairs),
 * dc_hip_xwide_pruned_order_dev the order of a pruned call.
 * The box rule of the pruned calls at these widths: a reference block is kept iff the squared gap of its box to the query
 * block's is below far2 = 1.0001 x max(r2, 2^-122) for r2 > 0 (far2 = 0, no block, otherwise) -- the floor of
 * dc_hip_populations_xwide_pruned_dev, not the bare 1.0001 x r2 of 65..256 columns: below about 0.37 FLT_MIN the canonical
 * sum of 1024 terms can round under a gap that 1.0001 x r2 already excludes.
 * Flagged data: the gated direct kernels answer on the original rows without a host synchronisation -- the generic
 * direct kernel up to 400 columns, the column-chunked one beyond --, counters (0, 0, 0).
 * No dc_variant value selects these calls; dc_hip_radius_pairs_dev, dc_hip_radius_min_edge[_segment]_dev,
 * dc_hip_radius_forest, the sessions and the CLI keep sending these widths to the direct kernels. */
DC_API int dc_hip_radius_pairs_xwide_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2, uint32_t* d_pops,
                                         uint32_t* d_pairs, size_t capacity, unsigned long long* d_count, void* d_ws,
                                         size_t ws_bytes, void* stream);
DC_API int dc_hip_radius_min_edge_xwide_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                            const uint32_t* d_comp, const uint32_t* d_rank, size_t segment,
                                            size_t n_segments, unsigned long long* d_best, uint32_t* d_pops, void* d_ws,
                                            size_t ws_bytes, void* stream);
DC_API int dc_hip_radius_forest_xwide(const float* coords, size_t n_rows, size_t n_cols, float r2, const uint32_t* rank,
                                      int device, uint32_t* edges, size_t* n_edges, uint32_t* n_rounds);
DC_API int dc_hip_radius_pairs_xwide_pruned_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                                uint32_t* d_pops, uint32_t* d_pairs, size_t capacity,
                                                unsigned long long* d_count, void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_radius_min_edge_xwide_pruned_dev(const float* d_coords, size_t n_rows, size_t n_cols, float r2,
                                                   const uint32_t* d_comp, const uint32_t* d_rank, size_t segment,
                                                   size_t n_segments, unsigned long long* d_best, uint32_t* d_pops,
                                                   void* d_ws, size_t ws_bytes, void* stream);
DC_API int dc_hip_radius_forest_xwide_pruned(const float* coords, size_t n_rows, size_t n_cols, float r2,
                                             const uint32_t* rank, int device, uint32_t* edges, size_t* n_edges,
                                             uint32_t* n_rounds);

/* the last wide sweep CALL in that workspace -- a self sweep (dc_hip_*_wide_dev, the radius graph included) or a cross sweep
 * (dc_hip_*_cross_wide_dev), the counters sit at the same place of either workspace: 32x32 tile pairs evaluated, MFMA instructions issued, frame pairs sent
 * to the exact path, summed over the launches of the call (a population call with more than 8 radii runs one launch
 * per 8: its counts are that multiple of a one-launch call's); all 0 when the direct kernels answered or there was
 * nothing to sweep.  The exact-pair count may differ by a few between runs of the same call (the column means are
 * summed in scheduling order; the results are not affected).  Any pointer may be NULL.  Synchronises the stream. */
DC_API int dc_hip_wide_info_dev(const void* d_ws, uint64_t* tiles, uint64_t* mfmas, uint64_t* exact_pairs,
                                void* stream);

/* free energies on ANOTHER array's scale: fe[i] = (float)-log((double)((float)pop[i] * (1.0f / (float)max_pop))),
 * with the device log + host-libm referee of dc_hip_free_energies_dev.  pop = 0 gives +inf, pop > max_pop a negative
 * value; max_pop = 0 is DC_ERR_INVALID_ARGUMENT.  Synchronises the stream. */
DC_API int dc_hip_free_energies_scaled_dev(const uint32_t* d_pops, size_t n, uint32_t max_pop, float* d_fe,
                                           void* stream);

/* ---- ASSIGNER: new frames to the states of a clustered reference, on either resident reference --------------------------
 * One call per batch for the job the two resident references exist for: every query's population in the reference at one
 * radius, its free energy on the reference's scale, its nearest reference frame, its nearest reference frame of lower
 * free energy, and its state: states_ref[hd] if hd exists, else states_ref[nn], else 0 (unassigned).  The values are those
 * of the handle's populations / dc_hip_free_energies_scaled_dev(max_pop) / the handle's nearest, bit for bit.
 * The free energies come from a table: a query's population against the reference is at most n_ref, so
 * table[p] = (float)-log((double)((float)p * (1.0f / (float)max_pop))), p = 0 .. n_ref, filled ONCE by the host libm when
 * the assigner is opened, holds every value dc_hip_free_energies_scaled_dev can give (+inf at 0, negative above max_pop).
 * A batch therefore needs no hand-off to the host: dc_hip_assign_batch_dev is five stream-ordered steps -- the handle's
 * stage, its populations, the table look-up, its nearest, the state pick -- and NOTHING in it synchronises with the host,
 * flagged batches included (the handles answer those behind their device-side gate).  A batch can be queued behind the one
 * before it and beside its own upload.
 * The assigner is a small host object.  It BORROWS the reference handle (which must hold its free energies and stay open)
 * and d_ws until it is closed, and d_query as the handle's stage does: until the batch's last step has run.  d_states_ref
 * is read by open (a copy is kept in the workspace) and not kept.  The table's host copy lives in the assigner until close,
 * so that its upload needs no synchronisation.  Calls on one assigner, and other calls on its handle, are ordered by the
 * caller: on one stream, or with synchronisation between them (a batch re-stages the handle).
 *   workspace_bytes  the table [n_ref + 1], the states [n_ref] and six arrays [max_batch] for the outputs a caller leaves
 *                    NULL; 0 for a zero count; monotone in each argument.  max_batch is the handle's
 *   open             max_pop: the scale of the free energies (the maximum of the reference's own populations); radius: the
 *                    one radius of every batch
 *   batch            n_query <= max_batch of the handle; 0 rows: DC_OK, nothing written.  d_states [n_query] is required;
 *                    d_pops, d_fe, d_nn_idx, d_nn_d2, d_hd_idx, d_hd_d2 [n_query] may each be NULL.  "none" is
 *                    (n_ref + 1, FLT_MAX).  The table index is clamped to n_ref
 * Refusals of open, all before a device is touched, dc_hip_last_error names the function, *out is NULL: a NULL handle,
 * array or `out`, a handle whose free energies were never set, max_pop == 0, a radius that is NaN or negative, a radius
 * whose fl32(r * r) exceeds the narrow handle's fl32(max_radius^2): DC_ERR_INVALID_ARGUMENT; a workspace smaller than
 * dc_hip_assign_workspace_bytes(n_ref, max_batch of the handle), or none: DC_ERR_WORKSPACE.  Of batch: a NULL assigner,
 * d_query or d_states, n_query > max_batch: DC_ERR_INVALID_ARGUMENT. */
typedef struct dc_assign dc_assign;
DC_API size_t dc_hip_assign_workspace_bytes(size_t n_ref, size_t max_batch);
DC_API int dc_hip_assign_open_dev(dc_reference* reference, const int32_t* d_states_ref, uint32_t max_pop, float radius,
                                  void* d_ws, size_t ws_bytes, void* stream, dc_assign** out);
DC_API int dc_hip_assign_open_wide_dev(dc_reference_wide* reference, const int32_t* d_states_ref, uint32_t max_pop,
                                       float radius, void* d_ws, size_t ws_bytes, void* stream, dc_assign** out);
/* ... on the resident reference of 257..1024 columns: the same call */
DC_API int dc_hip_assign_open_xwide_dev(dc_reference_xwide* reference, const int32_t* d_states_ref, uint32_t max_pop,
                                        float radius, void* d_ws, size_t ws_bytes, void* stream, dc_assign** out);
DC_API void dc_hip_assign_close(dc_assign* assign);
DC_API int dc_hip_assign_batch_dev(dc_assign* assign, const float* d_query, size_t n_query, int32_t* d_states,
                                   uint32_t* d_pops, float* d_fe, uint32_t* d_nn_idx, float* d_nn_d2, uint32_t* d_hd_idx,
                                   float* d_hd_d2, void* stream);

/* ---- ... and its host-pointer form, for C / C++ hosts and `clustering assign` -----------------------------------------------
 * All pointers are HOST pointers; the assigner owns its device memory, its streams and its pinned batch slots.  A
 * dc_assigner is used by one host thread at a time; the calling thread's current device is restored by every call.
 *   open       uploads the reference [n_ref][n_cols] and its states, runs the reference's self sweep at `radius` once
 *              (dc_hip_populations_dev under DC_VARIANT_AUTO; dc_hip_populations_wide_pruned_dev at 65..256 columns),
 *              dc_hip_free_energies_dev, then opens the resident reference of the width (max_batch, and for the narrow
 *              one max_radius = radius), sets its free energies and opens the assigner above.  ANY width is served: rows
 *              wider than 256 columns, and a reference the narrow handle refuses as too large, go through the per-call
 *              entry points (dc_hip_populations_cross_dev / dc_hip_nearest_neighbors_cross_dev, DC_VARIANT_AUTO) with the
 *              same table and pick kernels; that path makes no stream-order promise.  Rows of 257..1024 columns take the
 *              resident reference of those widths instead where the open call asks for it (dc_hip_assigner_open_flags,
 *              DC_ASSIGN_XWIDE=1: below).  Synchronises
 *   reference  the self sweep's populations [n_ref], free energies [n_ref] and maximum; any pointer may be NULL
 *   path       0 the narrow handle, 1 the wide handle, 2 the per-call cross entry points, 3 the resident reference of
 *              257..1024 columns (-1 for a NULL assigner)
 *   assign     any n_query, in chunks of max_batch through two batch slots: the upload of chunk k + 1 and the download of
 *              chunk k - 1 run on a copy stream, ordered by events, beside the sweeps of chunk k.  `states` [n_query] is
 *              required, the six other arrays [n_query] may be NULL; 0 rows: DC_OK.  Returns when every output is written.
 *              DC_ASSIGN_OVERLAP=0 (environment, read once per process: a measurement switch) puts copies and sweeps on
 *              one stream; the results are the same
 * Refusals of open, before a device is touched, *out is NULL: a NULL array or `out`, n_ref, n_cols or max_batch == 0, a
 * radius that is NaN or negative: DC_ERR_INVALID_ARGUMENT; counts beyond the cross calls' limits: DC_ERR_TOO_LARGE; then no
 * device: DC_ERR_NO_DEVICE; a device ordinal out of range: DC_ERR_INVALID_ARGUMENT. */
typedef struct dc_assigner dc_assigner;
DC_API int dc_hip_assigner_open(const float* ref, size_t n_ref, size_t n_cols, const int32_t* states_ref, float radius,
                                size_t max_batch, int device, dc_assigner** out);
/* dc_hip_assigner_open with flags.  DC_ASSIGNER_XWIDE_REFERENCE: at 257..1024 columns the reference's self sweep is
 * dc_hip_populations_xwide_pruned_dev and the batches go through the resident reference of those widths
 * (dc_hip_reference_xwide_*, dc_hip_assign_open_xwide_dev): dc_hip_assigner_path returns 3, every output equals path 2's
 * bit for bit.  A failure of that handle's open is returned (only the narrow handle's DC_ERR_TOO_LARGE falls back to
 * path 2).  Outside those widths the flag changes nothing.  Unknown bits: DC_ERR_INVALID_ARGUMENT, before a device is
 * touched.  WITHOUT the flag these widths stay on path 2, the direct kernels.
 * dc_hip_assigner_open is flags = 0, unless the environment holds DC_ASSIGN_XWIDE=1, which sets
 * DC_ASSIGNER_XWIDE_REFERENCE (read at every open: the hosts that call the old entry point, `clustering assign` among
 * them, opt in). */
#define DC_ASSIGNER_XWIDE_REFERENCE 0x1u
DC_API int dc_hip_assigner_open_flags(const float* ref, size_t n_ref, size_t n_cols, const int32_t* states_ref, float radius,
                                      size_t max_batch, int device, unsigned flags, dc_assigner** out);
DC_API int dc_hip_assigner_reference(const dc_assigner* assigner, uint32_t* pops_ref, float* fe_ref, uint32_t* max_pop);
DC_API int dc_hip_assigner_path(const dc_assigner* assigner);
DC_API int dc_hip_assigner_assign(dc_assigner* assigner, const float* queries, size_t n_query, int32_t* states,
                                  uint32_t* pops, float* fe, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx, float* hd_d2);
DC_API void dc_hip_assigner_close(dc_assigner* assigner);

/* ---------------------------------------------------------------------------------------
 * host-pointer entry points (mirror the reference's per-GPU host functions)
 * ------------------------------------------------------------------------------------- */

/* replaces calculate_populations_per_gpu(coords, n_rows, n_cols, radii, i_from, i_to, i_gpu)
 * (density_clustering_cuda.cu:45-52; declared as calculate_populations_partial in
 * density_clustering_cuda.hpp:21-30).  pops: HOST [n_radii*n_rows] uint32. */
DC_API int dc_hip_populations(const float* coords, size_t n_rows, size_t n_cols, const float* radii,
                              size_t n_radii, size_t i_from, size_t i_to, int device, uint32_t* pops);

/* replaces nearest_neighbors_per_gpu(coords, n_rows, n_cols, free_energy, i_from, i_to, i_gpu)
 * (density_clustering_cuda.cu:184-191).  All outputs HOST [n_rows].  Free energies may be any floats: "lower" is
 * the IEEE comparison fe[j] < fe[i], so a NaN is never lower and a NaN frame has no lower neighbour, and -0.0 is not
 * lower than +0.0. */
DC_API int dc_hip_nearest_neighbors(const float* coords, size_t n_rows, size_t n_cols, const float* fe,
                                    size_t i_from, size_t i_to, int device, uint32_t* nn_idx,
                                    float* nn_d2, uint32_t* hd_idx, float* hd_d2);

/* host-pointer forms of the cross sweeps (synchronous, one device, DC_VARIANT_AUTO).  pops HOST [n_radii][n_query];
 * neighbour outputs HOST [n_query]; fe_query == NULL: nn only. */
DC_API int dc_hip_populations_cross(const float* query, size_t n_query, const float* ref, size_t n_ref, size_t n_cols,
                                    const float* radii, size_t n_radii, size_t i_from, size_t i_to, int device,
                                    uint32_t* pops);
DC_API int dc_hip_nearest_neighbors_cross(const float* query, size_t n_query, const float* ref, size_t n_ref,
                                          size_t n_cols, const float* fe_query, const float* fe_ref, size_t i_from,
                                          size_t i_to, int device, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx,
                                          float* hd_d2);

/* host-pointer form of dc_hip_radius_pairs_dev.  pairs: HOST [capacity][2]; *count: pairs found (if
 * larger than capacity, call again with a buffer of that size). */
DC_API int dc_hip_radius_pairs(const float* coords, size_t n_rows, size_t n_cols, float r2, int device,
                               uint32_t* pairs, size_t capacity, unsigned long long* count);

/* bottleneck spanning forest of the radius graph: Boruvka rounds of dc_hip_radius_min_edge_dev with
 * the components merged on the host.  For every t the pairs of the forest with max(rank) < t connect
 * exactly the frames that the pairs of the full graph with max(rank) < t connect -- what a screening
 * threshold asks for -- with at most n_rows-1 pairs instead of all of them (9e8 at C3).
 *   rank     HOST [n_rows]: permutation of 0..n_rows-1
 *   edges    HOST [n_rows-1][2] uint32, out: frame ids of the forest's pairs
 *   n_edges  out: number of pairs written;  n_rounds (may be NULL): sweeps that were run */
DC_API int dc_hip_radius_forest(const float* coords, size_t n_rows, size_t n_cols, float r2,
                                const uint32_t* rank, int device, uint32_t* edges, size_t* n_edges,
                                uint32_t* n_rounds);

/* whole path on n_devices GPUs of this process (devices 0..n_devices-1; <= 0: all): ONE session (below)
 * -- open, populations, free energies of radius index fe_radius_index, neighbours, close.  Replaces the
 * pair CUDA::calculate_populations / CUDA::nearest_neighbors (density_clustering_cuda.cu:139-182,
 * :286-328), which upload the coordinates twice and merge every partial result on the host.
 * pops HOST [n_radii*n_rows]; fe, nn_*, hd_* HOST [n_rows] (fe may be NULL if nn_idx is; NN skipped if
 * nn_idx == NULL). */
DC_API int dc_hip_density_all(const float* coords, size_t n_rows, size_t n_cols, const float* radii,
                              size_t n_radii, size_t fe_radius_index, int n_devices, uint32_t* pops,
                              float* fe, uint32_t* nn_idx, float* nn_d2, uint32_t* hd_idx,
                              float* hd_d2);

/* ---------------------------------------------------------------------------------------
 * sessions: a trajectory resident on the GPUs across the phases of density_clustering.cpp:597-817
 * ------------------------------------------------------------------------------------- */
/* The reference's GPU host code allocates, uploads the coordinates and frees again inside every call
 * (density_clustering_cuda.cu:65-81, :133-135, :201-225, :278-281) and merges per-GPU partials on the
 * host (:171-180, :311-326).  A session uploads once per device and keeps coordinates, operand
 * workspace, populations, free energies and neighbours in HBM; one host thread drives each device
 * (like :152-157, :295-299); with more than one device the partial results merge ON the devices with
 * RCCL over xGMI -- all-reduce(sum, uint32) of the [n_radii][n_rows] populations, all-reduce(min,
 * uint64) of the packed neighbour words and of the forest's candidates -- and only final arrays cross
 * PCIe, from device 0.  Every device answers for one segment (dc_hip_*_segment_dev).  Host output
 * pointers may be NULL (the result then only stays resident for the next phase).  A session is used
 * by one host thread at a time. */
typedef struct dc_hip_session dc_hip_session;

/* devices: n_devices device ordinals, or NULL for 0..n_devices-1; n_devices <= 0: all devices.
 * coords: HOST, read during the call only.  RCCL (librccl.so.1) is loaded on first need, i.e. when a
 * session spans more than one device; if it cannot be loaded or its communicator cannot be built the
 * session merges its partials through the HOST instead, exactly like the reference
 * (density_clustering_cuda.cu:171-180, :311-326): same results, PCIe instead of xGMI.
 * Environment: DC_SESSION_MERGE=host forces the host merge, =rccl makes a missing RCCL an error.
 * The calling thread's current device is restored by every session entry point. */
DC_API int dc_hip_session_open(const float* coords, size_t n_rows, size_t n_cols, const int* devices,
                               int n_devices, dc_hip_session** session);
/* dc_hip_session_open with flags.  DC_SESSION_WIDE_SWEEPS: a session of 65..256 columns runs the pruned matrix-core
 * sweeps of those widths instead of the direct kernels -- populations: dc_hip_populations_wide_pruned_dev; neighbours:
 * dc_hip_nearest_neighbors_wide_pruned_dev, several devices merging by the all-gather of
 * dc_hip_neighbors_block_pack_wide_dev blocks (DC_SESSION_NN_MERGE=allreduce: by the minimum of packed words); pair
 * list: dc_hip_radius_pairs_wide_pruned_dev on device 0; forest: a dc_hip_radius_min_edge_wide_pruned_dev round per
 * device -- device g of G taking segment g of G.  Same results, same rules for every call; dc_hip_session_counters
 * then reports the evaluated tile pairs of dc_hip_wide_info_dev, summed over the devices (0 on flagged data).  Outside
 * 65..256 columns the flag changes nothing.  Unknown bits: DC_ERR_INVALID_ARGUMENT.
 * dc_hip_session_open is flags = 0, unless the environment holds DC_SESSION_WIDE=1, which sets DC_SESSION_WIDE_SWEEPS
 * (hosts that open their session through it -- the command line, the C++ shim, dc_hip_density_all). */
#define DC_SESSION_WIDE_SWEEPS 0x1u
DC_API int dc_hip_session_open_flags(const float* coords, size_t n_rows, size_t n_cols, const int* devices,
                                     int n_devices, unsigned flags, dc_hip_session** session);
/* 1: the session runs the wide sweeps (the flag is set and 65 <= n_cols <= 256); else 0 */
DC_API int dc_hip_session_wide(const dc_hip_session* session);
DC_API void dc_hip_session_close(dc_hip_session* session);
DC_API int dc_hip_session_devices(const dc_hip_session* session);      /* number of devices */
DC_API int dc_hip_session_uses_rccl(const dc_hip_session* session);    /* 1 if partials merge over RCCL */
/* 0: one device, nothing to merge; 1: RCCL collectives on the devices; 2: through the host */
DC_API int dc_hip_session_merge_mode(const dc_hip_session* session);
/* one line saying which merge this session runs and, for the host merge of a multi-device session, WHY RCCL is not
 * used (library not loadable, communicator not built, DC_SESSION_MERGE=host, duplicate devices) -- the reference's
 * merge (density_clustering_cuda.cu:152-180) is never silent about what it does, and a multi-GPU run that fell back
 * to PCIe is correct and slow: the C++ shim prints this line to stderr for mode 2, the command line under -v.
 * The string lives as long as the session. */
DC_API const char* dc_hip_session_merge_note(const dc_hip_session* session);
/* 32x32 frame-pair tiles the last population call / neighbour call evaluated, summed over devices */
DC_API int dc_hip_session_counters(const dc_hip_session* session, uint64_t* pop_tiles, uint64_t* nn_tiles);

/* CUDA::calculate_populations (density_clustering_cuda.cu:139-182) on the resident coordinates:
 * populations for n_radii radii, in the order given.  pops: HOST [n_radii*n_rows] or NULL. */
DC_API int dc_hip_session_populations(dc_hip_session* session, const float* radii, size_t n_radii,
                                      uint32_t* pops);
/* calculate_free_energies (density_clustering.cpp:197-212) of the resident populations of radius index
 * radius_index, on every device.  fe: HOST [n_rows] or NULL; max_pop: optional. */
DC_API int dc_hip_session_free_energies(dc_hip_session* session, size_t radius_index, float* fe,
                                        uint32_t* max_pop);
/* free energies from the caller instead (-D re-use, density_clustering.cpp:600-611; and the reference's
 * nearest_neighbors(coords, ..., free_energy) signature).  fe: HOST [n_rows], any floats, compared as
 * dc_hip_nearest_neighbors does (IEEE fe[j] < fe[i]: NaN is never lower, -0.0 not lower than +0.0).  A session of
 * 0 rows takes fe == NULL, as every other entry point takes its arrays of no rows. */
DC_API int dc_hip_session_set_free_energies(dc_hip_session* session, const float* fe);
/* CUDA::nearest_neighbors (density_clustering_cuda.cu:286-328) from the resident free energies, and
 * compute_sigma2 (density_clustering.cpp:334-343: double sum in frame order).  All outputs HOST
 * [n_rows] or NULL; sigma2 optional. */
DC_API int dc_hip_session_nearest_neighbors(dc_hip_session* session, uint32_t* nn_idx, float* nn_d2,
                                            uint32_t* hd_idx, float* hd_d2, double* sigma2);
/* dc_hip_radius_pairs on the resident coordinates (device 0 of the session). */
DC_API int dc_hip_session_radius_pairs(dc_hip_session* session, float r2, uint32_t* pairs, size_t capacity,
                                       unsigned long long* count);
/* dc_hip_radius_forest on the resident coordinates; with several devices every Boruvka round is one
 * segment sweep per device + one all-reduce(min, uint64) of the per-component candidates. */
DC_API int dc_hip_session_radius_forest(dc_hip_session* session, float r2, const uint32_t* rank,
                                        uint32_t* edges, size_t* n_edges, uint32_t* n_rounds);

#ifdef __cplusplus
}
#endif
#endif /* DC_DENSITY_H */
