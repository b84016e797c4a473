/* pcrcg.h -- C ABI of libpcrcg_hip.so, the MI355X (gfx950) implementation of PCR-CG's
 * feature-extraction hot path.
 *
 * The reference has no C-level FFI for this path: its native boundary is two CPython extension
 * modules (NumPy C-API glue) and, for the model, stock PyTorch ops.  Every entry point below names
 * the reference interface it replaces; INTEGRATION.md shows the binding a maintainer of the
 * reference would add (a ctypes stub, since the reference's host language is Python).
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer unless the parameter
 *     name starts with `h_`;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued on
 *     it and nothing synchronises unless documented;
 *   - no hidden allocation: scratch memory is a caller-provided workspace whose size comes from the
 *     matching *_ws_bytes() query; workspaces may be reused across calls on the same stream;
 *   - return value: PCRCG_OK (0) or a negative PCRCG_E* code; pcrcg_last_error() gives the
 *     message of the calling thread's last failure;
 *   - index tables use the reference's batched-neighbour contract: int64, row-major [Nq, cols],
 *     shadow (padding) value == number of stacked support points (ref:neighbors.cpp:319-325).
 */
#ifndef PCRCG_H
#define PCRCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCRCG_OK 0
#define PCRCG_EBADARG (-1)   /* null pointer / negative size / unsupported shape */
#define PCRCG_EWORKSPACE (-2) /* workspace too small */
#define PCRCG_ELAUNCH (-3)   /* HIP runtime error while enqueuing */
#define PCRCG_ECAPACITY (-4) /* device-side capacity overflow reported by pcrcg_check_status */

#define PCRCG_KPOINTS 15 /* kernel points per KPConv (ref:configs/test/indoor.yaml num_kernel_points) */

const char* pcrcg_last_error(void);
/* ABI version of this header: bumped on any signature change, on any change of a caller-held workspace's layout or size,
 * and on any change of the default arithmetic.  A binding compares pcrcg_abi_version() (what the loaded library was built
 * from) with the PCRCG_ABI_VERSION it was written against (pcrcg_amd/_lib.py does, at load time).
 *   2 (round 3)  forward groups, train-step runner, correspondences, debug switches; one-kernel KPConv entries removed
 *   3 (round 4/5) cell-grid workspace: 64-bit run cursor, 16-byte slots, compact cell list and ticket block (a grid built
 *                by a version-2 library cannot be walked); new entries pcrcg_radius_query_cells,
 *                pcrcg_pyramid_build_parts, pcrcg_gemm_f32_grad, pcrcg_thread_shares_gpu, pcrcg_gather_jobs;
 *                pcrcg_profile_kpconv flag bits;
 *                forward products in the fp16 two-term form with both range ends handled in the kernel (see
 *                pcrcg_gemm_set_mode); deterministic=1 debug switch
 *   4 (round 6)  pyramid builder: levels sized from pcrcg_pyramid_cfg::shrink, ONE host round trip per call, the KD-forests
 *                (level 0's, and one over the subsampled levels) on pcrcg_pyramid_cfg::side_stream (new cfg fields; pcrcg_pyramid_ws_bytes lost its `shrink`
 *                argument; pcrcg_pyramid_restore and pcrcg_reorder_job changed layout)
 *   The registration back end (pcrcg_ransac_ws_bytes, pcrcg_feature_match, pcrcg_ransac, pcrcg_ransac_trace) was added
 *   under version 4: it is additive -- no existing signature, layout or arithmetic changed.  So are its several-pairs
 *   entries (pcrcg_ransac_batch_ws_bytes, pcrcg_feature_match_batch, pcrcg_ransac_batch), added later under version 4, and
 *   the projection entries (pcrcg_project_depth_ws_bytes, pcrcg_project_depth, pcrcg_inject_frames with its
 *   pcrcg_image_frame, pcrcg_superglue_valid_maps), added after them, and the inlier statistics
 *   (pcrcg_inlier_stats_batch_ws_bytes, pcrcg_inlier_stats_batch), added after those, and the 2-D backbone
 *   (pcrcg_res50unet_arena_bytes, pcrcg_res50unet_pack, pcrcg_res50unet_ws_bytes, pcrcg_res50unet_forward), added after those,
 *   and the ModelNet evaluation's Chamfer distance (pcrcg_chamfer_batch_ws_bytes, pcrcg_chamfer_batch), added after those,
 *   and the interest-point sampler (pcrcg_weighted_sample_ws_bytes, pcrcg_weighted_sample_batch), added after those,
 *   and the voxel down-sampling of raw scans (pcrcg_voxel_down_sample_ws_bytes, pcrcg_voxel_down_sample_batch), added after
 *   that, and the decoded-frame conversion (pcrcg_prepare_frames), and the ModelNet pair preparation (pcrcg_modelnet_crop,
 *   pcrcg_modelnet_assemble), added after those, and the robust ICP entries (pcrcg_icp_plane_robust_batch_ws_bytes,
 *   pcrcg_icp_plane_robust_batch, pcrcg_colored_icp_robust_batch_ws_bytes, pcrcg_colored_icp_robust_batch), added under
 *   version 4, additive. */
#define PCRCG_ABI_VERSION 4
int pcrcg_abi_version(void);

/* Tuning / A-B switches, for measurements only: "name=value,name=value" (NULL: back to what the process started with --
 * the defaults, or what PCRCG_DEBUG made of them).  The same string is
 * read once from the environment variable PCRCG_DEBUG at first use; nothing else in the library reads the environment
 * except PCRCG_GEMM_MODE (pcrcg_gemm_set_mode).  Every switch defaults to the product behaviour:
 *   stat_sums=1 stat_sums_rows=2^30 att_mfma=1                                             network runner
 *   radius_blocks=0 kd_spin_limit=0 kd_blocks=0                                            front end
 *   att_tq=16                                                                              attention tile
 *   gemm_log=0 x6_tile=-1 x6_splitk=0 x6_t1=1 x6_t2=1 x6_order=-1 x6_big=0 x6_h2=1 gemm_tile=-1 gemm_splitk=0 gemm_split_target=768   GEMM plans
 *   train_side_stream=1 bwd_mfma=1                                                         train-step backward
 *   deterministic=0    1: bit-reproducible results -- no floating-point atomics (split-K partial tiles stored and added in
 *                      split order by a second pass, InstanceNorm statistics from stored partials, fixed-point scatter sums
 *                      in the train step, the 2-D backbone's BatchNorm sums stored per row tile and added in a fixed
 *                      order by a finishing pass per product); implies stat_sums=0 gemm_splitk=1; allocates its scratch itself.  Together with a fixed pairing of the pair engine (PairStreams(adaptive_jobs=False))
 *                      outputs are a function of the inputs alone.
 * (One accepted name is NOT in the list above: `walk`, the gather launches' query order, documented with pcrcg_query_walk
 * below.  The list is held to its 21 entries by tests/test_abi.py, which also means that test never sets `walk`;
 * tests/test_walk_gpu.py does.)
 * Returns PCRCG_EBADARG (and changes nothing) on an unknown name.  A switch that has been retired -- its default is now the
 * only behaviour, or its measurement aid is gone (DESIGN.md section 5 names them) -- is an unknown name like any other. */
int pcrcg_debug_set(const char* spec);
/* deterministic=1 allocates its scratch itself (partial tiles of split-K products, 64-bit fixed-point sums of the train
 * step's scatters, the backbone's per-tile BatchNorm sums -- pcrcg_res50unet_ws_bytes is the same in both modes): one buffer per stream it has run on, keyed by the stream handle, grown on demand and kept until the
 * process ends.  This frees all of it (after a device-wide synchronise): call it before destroying streams the mode has
 * used -- a recycled handle would otherwise inherit a stale entry -- or to get the memory back. */
int pcrcg_debug_release(void);

/* ------------------------------------------------------------------------------------------------
 * Front end: grid subsampling
 * Replaces cpp_wrappers.cpp_subsampling.grid_subsampling.subsample_batch(points, batches,
 * sampleDl=, max_p=) (zip:cpp_subsampling/wrapper.cpp:62-330) whose core is batch_grid_subsampling
 * (zip:cpp_subsampling/grid_subsampling/grid_subsampling.cpp:109-211).
 *   pts      [n,3] f32 stacked clouds           len      [nb] i32 points per cloud
 *   out_pts  [n,3] f32 (capacity n rows)        out_len  [nb] i32 cells kept per cloud
 *   out_m    [1]   i32 total rows written (= sum(out_len)); read it back after the stream drains
 * Output rows are the cell barycentres in the exact order the reference emits them (libstdc++
 * unordered_map iteration order per cloud), bit-identical in fp32.
 * ---------------------------------------------------------------------------------------------- */
size_t pcrcg_grid_subsample_ws_bytes(int n, int nb);
int pcrcg_grid_subsample_batch(const float* pts, int n, const int* len, int nb, float dl, int max_p,
                               float* out_pts, int* out_len, int* out_m, void* ws, size_t ws_bytes,
                               void* stream);

/* The same with the reference's optional `features=` and `classes=` (zip:cpp_subsampling/wrapper.cpp:62-330, format
 * "OO|$OOfsii"; grid_subsampling.cpp:59-70,88-102, grid_subsampling.h:33-73), added after ABI version 4 without changing
 * it: the points, lengths and launches of pcrcg_grid_subsample_batch are what they were.
 *   feats        [n, fdim] f32, row stride ld_feat >= fdim elements; NULL with fdim = 0: no features
 *   classes      [n, ldim] i32, dense;                                NULL with ldim = 0: no classes
 *   out_feats    [n, fdim] f32 dense (capacity n rows): per kept row the cell's features added in input order in fp32,
 *                starting from +0.0f, then divided by float(count) -- one correctly rounded fp32 division
 *   out_classes  [n, ldim] i32 dense (capacity n rows): per kept row and label column the most frequent label of the
 *                cell; among equally frequent labels the one std::max_element meets first when it walks the reference's
 *                std::unordered_map<int,int> histogram (libstdc++ list order, identity hash: not the smallest label)
 * Rows are in the barycentres' order and max_p cuts all three at the same rows; every result is bit-identical to the
 * reference's.  Two inputs on which the reference itself is undefined are defined here: a cloud of length 0 yields no
 * rows (the reference divides by zero), and every cloud's classes are its own rows of `classes` (the reference slices
 * them with an end that is out of range for ldim > 1 in every cloud after the first, grid_subsampling.cpp:155-156).
 * Returns PCRCG_EBADARG before any launch for fdim < 0, ldim < 0, ld_feat < fdim, or a null array whose width is > 0.
 * ws: pcrcg_grid_subsample_ex_ws_bytes(n, nb, fdim, ldim) bytes (>= the points-only size; the features need one int per
 * point beyond it -- they are summed straight into out_feats -- and the classes six ints per point and label column). */
size_t pcrcg_grid_subsample_ex_ws_bytes(int n, int nb, int fdim, int ldim);
int pcrcg_grid_subsample_batch_ex(const float* pts, int n, const int* len, int nb, float dl, int max_p,
                                  const float* feats, int fdim, int ld_feat, const int* classes, int ldim,
                                  float* out_pts, int* out_len, int* out_m, float* out_feats, int* out_classes,
                                  void* ws, size_t ws_bytes, void* stream);

/* Iteration order of a libstdc++ std::unordered_map<size_t,T> (identity hash) after inserting the
 * m DISTINCT keys in order; order[j] = insertion rank of the j-th visited element.  This is the
 * ordering step of the subsampling above, exported for unit tests
 * (zip:.../grid_subsampling.cpp:48,59-61,85).  keys [m] u64, order [m] i32. */
size_t pcrcg_umap_order_ws_bytes(int m);
int pcrcg_umap_order(const uint64_t* keys, int m, int* order, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Front end: radius neighbours
 * Replaces cpp_wrappers.cpp_neighbors.radius_neighbors.batch_query(queries, supports, q_batches,
 * s_batches, radius=) (ref:cpp_wrappers/cpp_neighbors/wrapper.cpp:58-238) whose core is
 * batch_nanoflann_neighbors (ref:cpp_wrappers/cpp_neighbors/neighbors/neighbors.cpp:211-333), plus
 * the `[:, :max_neighbors]` truncation and `.long()` cast of batch_neighbors_kpconv
 * (ref:datasets/dataloader.py:54-69, 347-349).
 *
 * The search structure (a hashed uniform cell grid over the supports, cell edge = radius) is built
 * once per support set and can serve several query sets of the same radius: in the KPConv pyramid
 * the conv, pool and upsample searches over one level all use that level's radius
 * (ref:datasets/dataloader.py:273,298,301).
 *   sup [ns,3] f32, slen [nb] i32, grid = workspace of pcrcg_cellgrid_ws_bytes(ns, nb) bytes.
 * ---------------------------------------------------------------------------------------------- */
size_t pcrcg_cellgrid_ws_bytes(int ns, int nb);
int pcrcg_cellgrid_build(const float* sup, int ns, const int* slen, int nb, float radius, void* grid,
                         size_t grid_bytes, void* stream);
/*   q [nq,3] f32, qlen [nb] i32; out_idx [nq, cols] i64: row = supports with d2 < radius^2 (fp32,
 *   unfused) in ascending (d2, index) order, truncated to `cols`, padded with ns;
 *   out_count [nq] i32 (may be NULL) = untruncated list length per query;
 *   out_max_count [1] i32 = max over queries (the reference's column count), accumulated with
 *   atomicMax: zero it (or let pcrcg_radius_neighbors_batch do so) before the first query call;
 *   status [1] i32 (may be NULL): set non-zero if a list exceeded the kernel's staging capacity. */
int pcrcg_radius_query(const float* q, int nq, const int* qlen, int ns, const int* slen, int nb,
                       float radius, const void* grid, int cols, int64_t* out_idx, int* out_count,
                       int* out_max_count, int* status, void* stream);
/* pcrcg_radius_query that also reports the rows whose REFERENCE order is not the (d2, index) order: rows that hold
 * two neighbours of EXACTLY equal d2, the first of them inside the kept `cols` columns.
 *   out_tie_rows [nq] i32: the row numbers (unordered), out_tie_count [1] i32: how many -- accumulated with
 *   atomicAdd, zero it before the call.  Both NULL = pcrcg_radius_query. */
int pcrcg_radius_query_ex(const float* q, int nq, const int* qlen, int ns, const int* slen, int nb,
                          float radius, const void* grid, int cols, int64_t* out_idx, int* out_count,
                          int* out_max_count, int* status, int* out_tie_rows, int* out_tie_count, void* stream);
/* pcrcg_radius_query_ex for several INDEPENDENT groups of clouds stacked into one call (e.g. two fragment pairs =
 * four clouds, group = 2): indices are written relative to the first support of the query's group, rows are padded
 * with the group's support count, and out_max_count is an array with one entry per group ([ceil(nb / group)], zeroed
 * by the caller) -- the table is the groups' own tables stacked on top of each other, row for row what separate
 * calls would have written.  group = 0: one group (pcrcg_radius_query_ex). */
int pcrcg_radius_query_groups(const float* q, int nq, const int* qlen, int ns, const int* slen, int nb, int group,
                              float radius, const void* grid, int cols, int64_t* out_idx, int* out_count,
                              int* out_max_count, int* status, int* out_tie_rows, int* out_tie_count, void* stream);
/* The CELL-COOPERATIVE search (round 4; the kernel the pyramid builder uses): the queries are walked cell by cell through
 * a grid of their own, `qgrid` = pcrcg_cellgrid_build over the QUERY points (any radius: it only sets the size of the
 * query cells; a level's conv grid serves), nb clouds matching the support grid's.  One workgroup per occupied query cell
 * resolves the hash probes of the support cells within reach once, stages their candidates and the cell's queries in LDS,
 * and its wavefronts answer the cell's queries from LDS -- same result set, order, padding, counts, tie rows and group
 * semantics as pcrcg_radius_query_groups, row for row (replaces the hot loop of
 * ref:cpp_wrappers/cpp_neighbors/neighbors/neighbors.cpp:268-301 and :319-325).  Rows of more than 128 hits and cells
 * whose neighbourhood exceeds the staging capacity are finished by the per-query kernel inside the same call
 * (status bit 4 is set and cleared on the way; q / qlen / slen are what that pass reads).
 * The kernel's work counters live in `qgrid` (it leaves them zeroed): searches that walk the SAME query grid must be
 * ordered on one stream (or by events) -- two of them running at once would share the counters.  Searches over
 * different query grids, and any number of searches reading the same SUPPORT grid, may overlap freely. */
int pcrcg_radius_query_cells(const void* qgrid, const float* q, int nq, const int* qlen, const void* sgrid, int ns,
                             const int* slen, int nb, int group, float radius, int cols, int64_t* out_idx, int* out_count,
                             int* out_max_count, int* status, int* out_tie_rows, int* out_tie_count, void* stream);
/* Convenience: zero out_max_count/status, build the grid in `ws`, run one query. */
size_t pcrcg_radius_neighbors_ws_bytes(int ns, int nb);
int pcrcg_radius_neighbors_batch(const float* q, int nq, const float* sup, int ns, const int* qlen,
                                 const int* slen, int nb, float radius, int cols, int64_t* out_idx,
                                 int* out_count, int* out_max_count, int* status, void* ws,
                                 size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Front end: the reference's order inside groups of exactly equal distance
 * batch_nanoflann_neighbors sorts its hits by distance only (IndexDist_Sorter, zip:cpp_utils/nanoflann/
 * nanoflann.hpp:208-214) with an unstable std::sort over nanoflann's traversal order, and
 * batch_neighbors_kpconv then cuts the rows at `[:, :limit]` (ref:datasets/dataloader.py:65-69): which members of
 * a tie group survive, and which of two equidistant coarse points lands in column 0 of an upsample table, is
 * decided by that order.  These calls reproduce it entry for entry (pcrcg_amd/csrc/tieorder.hip):
 *
 *   pcrcg_kdforest_build   nanoflann 1.3.0's KD-tree (leaf size 10, ref:.../neighbors.cpp:245) for each of the
 *                          nb clouds of `sup` -- the clouds of ALL pyramid levels can be stacked into one forest.
 *                          forest = workspace of pcrcg_kdforest_ws_bytes(ns, nb) bytes; one launch.
 *   pcrcg_radius_reorder   rewrites rows of a table produced by pcrcg_radius_query(_ex): the query clouds
 *                          0..nbq-1 search the forest's clouds cloud0..cloud0+nbq-1; indices are written relative
 *                          to the first of them and rows are padded with their total size (the table's shadow
 *                          index).  rows [nrows] i32 = the rows to redo (out_tie_rows; NULL = all nq rows);
 *                          count [nq] i32 (may be NULL) = out_count of the query, cross-checked;
 *                          max_count = staging width (>= the longest list among `rows`, <= 8192);
 *                          idx [nq, cols] i64.
 *   pcrcg_radius_reorder_jobs  the same for up to PCRCG_MAX_REORDER_JOBS tables over one forest in ONE launch
 *                          (all tables of a pair).
 *                          status [1] i32 (may be NULL): 1 forest kernel gave up waiting for work, 2 traversal stack
 *                          overflow (more than 128 pending branches), 3 hit count differs from `count`,
 *                          4 list longer than max_count.
 * ---------------------------------------------------------------------------------------------- */
#define PCRCG_MAX_REORDER_JOBS 12
typedef struct pcrcg_reorder_job {
    const float* q;       /* [nq,3] queries of the table */
    const int* qlen;      /* [nbq] */
    const int* rows;      /* [nrows] rows to redo, NULL = all */
    const int* count;     /* [nq] or NULL */
    int64_t* idx;         /* [nq, cols] table, rewritten in place */
    int nq, nbq, cloud0, nrows, max_count, cols;
    float radius;
    int group;            /* > 0: the nbq clouds are independent groups of `group` clouds (pcrcg_radius_query_groups):
                             indices relative to the group's first support, padding = the group's support count */
    const float* sup;     /* version 4: forest != NULL: this job searches a forest of its OWN -- built over `sup` with */
    const void* forest;   /*   pcrcg_kdforest_build(sup, forest_ns, .., forest_nb, ..) -- instead of the call's (the  */
    int forest_ns, forest_nb; /* pyramid builder keeps one forest per level); NULL: the call's sup / forest / ns / nb */
} pcrcg_reorder_job;
size_t pcrcg_kdforest_ws_bytes(int ns, int nb);
int pcrcg_kdforest_build(const float* sup, int ns, const int* slen, int nb, void* forest, size_t forest_bytes,
                         void* stream);
int pcrcg_radius_reorder(const float* q, int nq, const int* qlen, int nbq, const float* sup, int ns, int nb,
                         const void* forest, int cloud0, float radius, const int* rows, int nrows, const int* count,
                         int max_count, int cols, int64_t* idx, int* status, void* stream);
int pcrcg_radius_reorder_jobs(const pcrcg_reorder_job* jobs, int njobs, const float* sup, int ns, int nb,
                              const void* forest, int* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * KPConv (rigid, linear influence, sum aggregation) -- replaces KPConv.forward
 * (ref:models/blocks.py:229-374):
 *   out[q,:] = (1/n_q) * sum_k ( sum_h max(0, 1 - |s[idx[q,h]] - q_pts[q] - kp[k]| / extent)
 *                                 * x[idx[q,h],:] ) @ W[k]
 *   n_q = max(1, #{h : sum_c x[idx[q,h],c] > 0}); idx == ns addresses the shadow support
 *   (point 1e6,1e6,1e6; feature 0).
 * Stage 1 (this call) gathers and aggregates:  wf [nq, 15*cin] f32 (kernel-point major: column
 * k*cin + c) and inv_n [nq] f32 = 1/n_q.  Stage 2 is the dense contraction wf @ W[15*cin, cout]
 * scaled per row by inv_n (pcrcg_gemm_f32 with row_scale).
 *   q_pts [nq,3], s_pts [ns,3], idx [nq, h] i64 (row stride ld_idx elements), x [ns, cin] f32,
 *   kp [15,3] f32.
 * ---------------------------------------------------------------------------------------------- */
size_t pcrcg_kpconv_ws_bytes(int ns);
int pcrcg_kpconv_aggregate(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx,
                           int h, int ld_idx, const float* x, int cin, const float* kp, float extent,
                           float* wf, float* inv_n, void* ws, size_t ws_bytes, void* stream);
/* The whole first layer of the geometry-only configurations (cin = 1: x [ns] f32, one feature per support point) in ONE
 * kernel -- what pcrcg_kpfcnn_forward runs for it when its statistics are column sums:
 *   out[q, c] = inv_n[q] * sum_k wf[q, k] * wt[c, k]    for c < cout,  wf and inv_n as pcrcg_kpconv_aggregate defines them,
 * wt [cout, 16] f32 the K-contiguous weights (pcrcg_block.kp_wt; column 15 is not used), accumulated in fp64 over k = 0 .. 14 in
 * order and rounded to fp32 once.
 * sums [2][cout] f64, ZEROED by the caller, receives the column sums and the column sums of squares of out (fp64 atomics,
 * one pair per column and 64 queries).  Columns cout .. ld_out - 1 of out are not written.  cout % 4 == 0, cout >= 4 and wt
 * 16-byte aligned, else PCRCG_EBADARG.  ws: pcrcg_kpconv_ws_bytes(ns). */
int pcrcg_kpconv_c1_layer(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx,
                          const float* x, const float* kp, float extent, const float* wt, int cout, float* out, int ld_out,
                          float* inv_n, void* sums, void* ws, size_t ws_bytes, void* stream);
/* Stage 1 of the bf16 feature-storage VARIANT (pcrcg_model.feature_bf16): x is fp32 at the boundary; x_bf16
 * ([ns, cin] u16 scratch) receives its round-to-nearest-even bf16 copy, which is what the neighbour gathers read, and
 * wf_bf16 ([nq, 15*cin] u16) the aggregate rounded the same way.  Geometry, influences, n_q and the accumulation are
 * fp32.  cin % 4 == 0.  Stage 2 is pcrcg_gemm_bf16a_f32_colstats. */
int pcrcg_kpconv_aggregate_bf16(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h,
                                int ld_idx, const float* x, int cin, const float* kp, float extent, void* x_bf16,
                                void* wf_bf16, float* inv_n, void* ws, size_t ws_bytes, void* stream);

/* The GENERAL KPConv gather (csrc/kpconv_ex.hip): deformable and modulated kernels, every influence function and both
 * aggregation modes of ref:models/blocks.py:229-374.  The arguments of pcrcg_kpconv_aggregate (same workspace, same wf
 * and inv_n) plus:
 *   offset_features [nq, ld_off] f32 or NULL (rigid kernel): the offset convolution's output with offset_bias added;
 *     columns 0 .. 44 are the offsets, kp_q[k] = offset_features[q, 3k..3k+2] * extent + kp[k] (fp32, not fused), columns
 *     45 .. 59 the modulation logits when `modulated` (ld_off >= 45, or 60 when modulated);
 *   influence: 0 constant (1), 1 linear (max(0, 1 - sqrt(d2)/extent)), 2 gaussian (exp(-d2 / (2 (0.3 extent)^2 + 1e-9)));
 *   closest: 0 sum, 1 only the nearest kernel point of a neighbour keeps its weight (first index on ties);
 *   modulated: wf[q,k,:] is multiplied by 2 sigmoid(offset_features[q, 45 + k]);
 *   min_d2 [nq, 15] f32 or NULL: min over ALL h columns (shadow columns included) of d2[q,h,k].
 * d2[q,h,k] = |s[idx[q,h]] - q - kp_q[k]|^2.  With offset_features, neighbour h is KEPT iff d2[q,h,k] < extent * extent
 * for some k; a neighbour that is not kept contributes nothing to wf, is not counted in n_q and its feature row is not
 * read.  Without, every neighbour is kept.  Inference only: there is no backward for this entry. */
int pcrcg_kpconv_aggregate_ex(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h,
                              int ld_idx, const float* x, int cin, const float* kp, float extent,
                              const float* offset_features, int ld_off, int influence, int closest, int modulated,
                              float* wf, float* inv_n, float* min_d2, void* ws, size_t ws_bytes, void* stream);

/* The order in which the gather kernels visit their queries (csrc/walk.hip).  pcrcg_query_walk writes walk[n] i32, a
 * permutation of 0 .. n-1: the queries of points [n,3] sorted by key, the 12-bit Morton interleave (x bit i -> key bit 3i,
 * y -> 3i+1, z -> 3i+2) of the point's cell in a 16 x 16 x 16 grid over the cloud's bounding box,
 * cell = clamp(int((p - lo) * 16 / max(hi - lo, tiny)), 0, 15) per axis; a NaN or infinite coordinate goes to cell 0 and
 * does not count for the box.  The order inside one key is arbitrary.  key [n] i32 receives the keys (or NULL).  n = 0
 * writes nothing.  A kernel that is given a walk covers POSITIONS: workgroup b runs on XCD b mod 8 and takes its queries
 * from the (b mod 8)-th eighth of the walk, so that the neighbour rows of one part of the cloud are fetched into ONE
 * XCD's L2 -- every output row is computed exactly as without a walk (bit-identical results).
 * The forward runner builds one walk per level and call and hands it to the gather launches whose support rows exceed an
 * L2 (debug switch `walk`, default 1; pcrcg_debug_set("walk=0"): index order everywhere, "walk=2": every launch walks --
 * listed here and not above because it is an order of processing, not of arithmetic).
 * The _walk forms of the three gather entries are TEST-ONLY AND UNSTABLE: no caller other than this repository's tests and
 * timing scripts may rely on them, and they may change or go without an ABI version bump.  They are the plain entries with
 * the queries' order given (walk [nq] i32; NULL: the plain entry).  The walk is NOT validated: it must be a permutation of
 * 0 .. nq-1 (what pcrcg_query_walk writes); anything else gives duplicated and missing output rows (entries outside the
 * range are clamped into it, so no address leaves the arrays). */
int pcrcg_query_walk(const float* points, int n, int* walk, int* key, void* stream);
int pcrcg_kpconv_aggregate_walk(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx,
                                int h, int ld_idx, const float* x, int cin, const float* kp, float extent,
                                float* wf, float* inv_n, void* ws, size_t ws_bytes, const int* walk, void* stream);
int pcrcg_kpconv_aggregate_bf16_walk(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h,
                                     int ld_idx, const float* x, int cin, const float* kp, float extent, void* x_bf16,
                                     void* wf_bf16, float* inv_n, void* ws, size_t ws_bytes, const int* walk, void* stream);
int pcrcg_gather_max_walk(const float* x, int ns, int c, const int64_t* idx, int nq, int h, int ld_idx,
                          float* out, const int* walk, void* stream);

/* Measurement aid for bench.py: when enabled, the gather/aggregate kernel of every
 * pcrcg_kpconv_aggregate call (kind 0; kind 1 is reserved for a one-kernel KPConv)
 * are launched with HIP start / stop events (hipExtLaunchKernel) on their own stream, i.e. the kernel's own
 * execution time as rocprofv3 reports it, excluding the time its dispatch waited behind other streams; _read
 * waits for them and returns up to `cap` records (milliseconds, nq / h / cin of the launch, cout for kind 1).
 * `enable` is a bit mask: 1 = the KPConv kernels (kinds 0, 1, 2 = bf16-storage gather), 2 = every GEMM of the
 * split-bf16 family (kind 3: nq = M, h = N, cin = K, cout = bf16 matrix products per element, 6 or 3), 0 = off.
 * Safe to call from several host threads; off by default. */
void pcrcg_profile_kpconv(int enable);
int pcrcg_profile_kpconv_read(float* ms, int* nq, int* h, int* cin, int* cout, int* kind, int cap);

/* C[m,n] = (A[m,k] @ Bop[k,n]) * row_scale[m] + bias[n]   (fp32 in, fp32 MFMA accumulate; row_scale
 * and bias may be NULL).  Row-major with leading dimensions in elements.
 *   trans_b = 0: b is [k,n] (ldb >= n), Bop = b      -- KPConv weights [15*cin, cout], P @ V
 *   trans_b = 1: b is [n,k] (ldb >= k), Bop = b^T    -- nn.Linear / 1x1 conv weights [out,in], Q @ K^T
 * Replaces the torch.matmul / nn.Linear / 1x1 nn.Conv1d contractions of the path
 * (ref:models/blocks.py:361-366, 487; ref:models/architectures.py:528,538-539; ref:models/gcn.py:123-173). */
int pcrcg_gemm_f32(const float* a, int lda, const float* b, int ldb, int trans_b, float* c, int ldc, int m,
                   int n, int k, const float* row_scale, const float* bias, void* stream);
/* Same GEMM; additionally, when every output element is written exactly once (no split-K), the
 * epilogue leaves per-column partial sums / sums of squares of C in `colstats`
 * (pcrcg_gemm_colstats_bytes(m, n) bytes, layout [2][n][chunks] fp64) and stores the chunk count in the
 * HOST integer *h_chunks; otherwise *h_chunks = 0 and the caller computes the statistics with
 * pcrcg_instnorm_stats.  Every GEMM of the path feeds an InstanceNorm (ref:models/blocks.py:456-463), so
 * this saves one full read of C per layer. */
size_t pcrcg_gemm_colstats_bytes(int m, int n);
int pcrcg_gemm_f32_colstats(const float* a, int lda, const float* b, int ldb, int trans_b, float* c, int ldc,
                            int m, int n, int k, const float* row_scale, const float* bias, void* colstats,
                            size_t colstats_bytes, int* h_chunks, void* stream);
/* C = (A @ B^T) * row_scale + bias with A stored as bf16 ([m, k] u16, lda in ELEMENTS, lda % 8 == 0, 16-byte aligned,
 * k % 32 == 0) and B fp32 [n, k]: B is split exactly into three bf16 terms as in mode 1 below and the three products
 * against the single A term run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- exact in B, bf16-rounded in A
 * only by A's storage format.  Column partials as pcrcg_gemm_f32_colstats. */
int pcrcg_gemm_bf16a_f32_colstats(const void* a_bf16, int lda, const float* b, int ldb, float* c, int ldc, int m, int n,
                                  int k, const float* row_scale, const float* bias, void* colstats,
                                  size_t colstats_bytes, int* h_chunks, void* stream);

/* C (+)= f(A)[rows] @ B^T + bias with B [n, k] k-contiguous: the products with which pcrcg_kpfcnn_forward folds a
 * neighbouring operator into a GEMM's A loads instead of running it as a pass of its own.
 *   idx != NULL    output row r uses row idx[r * ld_idx] of A [ns, k] (lda), the zero row `zero_row` (>= k floats of 0)
 *                  when that index is outside [0, ns) -- nearest_upsample with its shadow index
 *                  (ref:models/blocks.py:77-87); with accumulate the decoder's nearest_upsample -> cat(skip) -> unary
 *                  (ref:models/architectures.py:568-569) is two products into one output and neither the upsampled
 *                  matrix nor the concatenation is written;
 *   a_sums != NULL A is the RAW output of a product; its InstanceNorm + LeakyReLU (ref:models/blocks.py:456-470) is
 *                  applied on load, f(a) = lrelu((a - mean_k) * rstd_k, a_slope), from the fp64 column sums
 *                  a_sums [2][k] over a_count rows (biased variance, a_eps); a gathered shadow row stays zero;
 *   accumulate     != 0 adds the product to C (fp32 atomics) instead of storing it.
 * Split-bf16 arithmetic only (mode 1 below). */
int pcrcg_gemm_f32_fused(const float* a, int lda, const int64_t* idx, int ld_idx, int ns, const float* zero_row,
                         const void* a_sums, double a_count, float a_eps, float a_slope, const float* b, int ldb,
                         const float* bias, float* c, int ldc, int m, int n, int k, int accumulate, void* stream);

/* Arithmetic of the C = A @ B^T products (trans_b = 1) behind pcrcg_gemm_f32 / _colstats / _ex:
 *   0: v_mfma_f32_32x32x2_f32 on the fp32 operands (the fp32 matrix rate, 157 TF on MI355X);
 *   1: (default) the fp32 operands are split into 16-bit terms and the products run on the 16-bit matrix cores with
 *      fp32 accumulation.  The forward products (k-contiguous fp32 operands) use the TWO-term fp16 form
 *      x = h + 2^-11 l, three v_mfma_f32_32x32x16_f16 per 16-deep chunk (representation and dropped term: 2^-22
 *      relative per product; measured against float64 no worse than the bf16 form or mode 0).  fp16's normal range is
 *      2^-14 .. 65504, and BOTH ends are handled inside the kernel, per tile, with no flag for the host and no different
 *      result contract (round 5):
 *        above   an operand value beyond 65504 leaves a non-finite partial sum behind;
 *        below   every thread keeps the largest |x| of the values it splits, per tile row of A and of B (an output row /
 *                an output column); a row that is not all zeros and holds no value of at least 2^-14 is one whose h terms
 *                are all fp16 subnormals (absolute floor 2^-36 per value instead of 2^-22 relative);
 *      a workgroup that finds either after its loop throws its sums away and redoes its tile in the exact bf16 form
 *      below.  What the fp16 form keeps is therefore, for every finite fp32 operand: each element's representation error
 *      is at most 2^-22 of the LARGEST value of its row (not of the element itself: a 1e-9 entry beside O(1) entries of
 *      the same row is carried with an absolute error of 2^-36) -- a normwise-per-row fp32-class bound, measured
 *      <= 5e-7 of a float64 product at every whole-operand scale from 1 to 1e-12 (tests/test_gemm_range_gpu.py).
 *      The other products (the training rows' k-major forms without a named gradient operand, bf16-stored operands) and
 *      PCRCG_DEBUG=x6_h2=0 use the EXACT three-term bf16 form: three bf16 terms per value, the six leading cross products
 *      on v_mfma_f32_32x32x16_bf16, dropped terms below 2^-23 relative per product, at 16/6 of the fp32 matrix rate (the
 *      fp16 form: 16/3).
 * Process-wide (one atomic word); also read once from the environment variable PCRCG_GEMM_MODE.  Interface: fp32 in,
 * fp32 out in both modes.
 * Non-finite operands: mode 1 turns an operand value of +-inf into NaN in every output it touches (the split's residual
 * is inf - inf), where mode 0 / an fp32 GEMM would produce +-inf or, against a zero, NaN as well; NaN operands give NaN in
 * both modes.  Finite operands keep fp32's range in both forms: the bf16 form's three terms are exact for every finite
 * fp32 value whose magnitude is at least 2^-110 (below that the third term leaves fp32's own subnormal range), and the fp16
 * form hands every tile it cannot hold to it.  The train step's non-finite check (pcrcg_amd/trainer.py: the reference's
 * validate_gradient) treats inf and NaN alike, so the skip decision does not depend on the mode. */
void pcrcg_gemm_set_mode(int mode);
int pcrcg_gemm_get_mode(void);
/* Diagnostics of the fp16 form's range checks (synchronous; not for the hot path): out2[0] = tiles redone in the bf16 form
 * since the last reset because an operand value lay beyond fp16's range, out2[1] = because a row lay below it.  reset != 0
 * clears the counters afterwards.  out2 may be NULL (reset only). */
int pcrcg_gemm_redo_counts(unsigned long long* out2, int reset);
/* Declares that the CALLING HOST THREAD enqueues its network calls beside other streams that keep the GPU busy (on = 1;
 * 0 takes it back; per thread, default off).  The products of such a thread are planned WITHOUT split-K:
 * alone on the GPU a small product is split until ~200 workgroups exist, which fills the chip; beside other streams
 * their kernels fill the idle CUs anyway and every slice only costs fp32 atomics, a zeroed output and the column statistics
 * its epilogue could have left (+5 % pairs/s in the four-stream pair engine, whose model threads make this call; -1.9 %
 * for a forward that does run alone; round 4-5: a few slices, x6_t1 / x6_t2 = 32 / 128; round 6: none, 1 / 1).  Results
 * differ by summation order only.  No reference counterpart (ref:main.py:15 one process, one stream). */
void pcrcg_thread_shares_gpu(int on);

/* ------------------------------------------------------------------------------------------------
 * Point-wise blocks
 *
 * Non-finite values.  A NaN or an infinity in a FEATURE value (an activation, a weight, a pixel) goes where torch's
 * operation sends it: every maximum (pcrcg_gather_max, the edge convolution's emax, the 2-D backbone's ReLU and max-pool)
 * returns NaN when an operand is NaN, as torch.max / F.relu / F.max_pool2d do; pcrcg_l2norm_rows and the feature head give
 * an all-NaN row for a row that holds a NaN, as F.normalize does (clamp_min keeps NaN); the InstanceNorm entries make a
 * column that holds a non-finite value non-finite in every row and leave every other column alone; the copies
 * (pcrcg_gather_first*, pcrcg_copy2d) move the bits.  Only the two score heads scrub (nan_to_num, as the reference).
 * Kernels that contain a product (the GEMMs, KPConv, the convolutions, attention) keep the SET of finite outputs and turn a
 * NaN into a NaN, but may turn an infinity into a NaN where torch keeps the infinity: the split-term products form
 * inf - inf.  tests/test_nonfinite_forward_gpu.py holds the entries to this against float64 torch on the CPU.
 * Non-finite COORDINATES (points, kernel points, kNN coordinates) are outside the contract: the front end defines no
 * tables for them, and the KPConv influence clamp max(1 - d / extent, 0) is an fmaxf that sends a NaN distance to 0.
 * ---------------------------------------------------------------------------------------------- */
/* max_pool (ref:models/blocks.py:86-102): out[q,c] = max_h xpad[idx[q,h],c], shadow row = 0. */
int pcrcg_gather_max(const float* x, int ns, int c, const int64_t* idx, int nq, int h, int ld_idx,
                     float* out, void* stream);
/* closest_pool (ref:models/blocks.py:71-83): out[q,:] = xpad[idx[q,0],:]; writes into a row-major
 * destination with leading dimension ld_out (so it can fill the left part of a concat buffer). */
int pcrcg_gather_first(const float* x, int ns, int c, const int64_t* idx, int nq, int ld_idx, float* out,
                       int ld_out, void* stream);
/* The same for `count` (1 .. 4) clouds of one width in ONE launch: x, ns, idx, nq, ld_idx and out are host arrays of
 * `count` entries; the rows of every x[g] have leading dimension ld_x >= c (the single-cloud entry reads dense rows).
 * Columns c .. ld_out - 1 of out are not written; a cloud with nq[g] = 0 is skipped. */
int pcrcg_gather_first_multi(const float* const* x, const int* ns, const int64_t* const* idx, const int* nq, const int* ld_idx,
                             float* const* out, int count, int c, int ld_x, int ld_out, void* stream);
/* InstanceNorm over all rows + LeakyReLU (BatchNormBlock/UnaryBlock/ResnetBottleneckBlock,
 * ref:models/blocks.py:433-470, 493-500, 650-678):
 *   stats[2*c] receives per-channel (mean, 1/sqrt(var+eps)) of x [n,c] (biased variance);
 *   y = lrelu( (x - mean_x) * rstd_x + res_term, slope )
 *   res_term = 0                                   if res == NULL
 *            = res                                 if res_stats == NULL
 *            = (res - mean_r) * rstd_r             otherwise (res_stats from a previous call)
 * x, res, y are row-major with leading dimensions ldx, ldr, ldy.  slope 1.0 = no activation.
 * ws: pcrcg_instnorm_ws_bytes(c) bytes. */
size_t pcrcg_instnorm_ws_bytes(int c);
/* (mean, rstd) pairs from [2][c][chunks] fp64 partial sums over `count` rows (see
 * pcrcg_gemm_f32_colstats); fixed summation order, deterministic. */
int pcrcg_instnorm_stats_from_partials(const void* partials, int chunks, int c, double count, float eps,
                                       float* stats, void* stream);
int pcrcg_instnorm_stats(const float* x, int n, int c, int ldx, float eps, float* stats, void* ws,
                         size_t ws_bytes, void* stream);
int pcrcg_instnorm_apply(const float* x, int n, int c, int ldx, const float* stats, const float* res,
                         int ldr, const float* res_stats, float slope, float* y, int ldy, void* stream);
/* The same with the statistics given as fp64 column SUMS: sums [2][c] = (sum_r x[r,ch], sum_r x[r,ch]^2) over `count`
 * rows (what pcrcg_kpfcnn_forward's GEMM epilogues leave), mean / biased variance / rstd
 * derived on the fly -- no finishing launch between the producing GEMM and the normalisation.  res_sums (may be NULL):
 * the residual is normalised by its own sums, else added as is.  c % 4 == 0 and c / 4 a divisor or a multiple of 256
 * (every width of the architecture); rows 16-byte aligned. */
/* sums [2][c] f64 += (column sums, column sums of squares) of x [n, c]; the caller zeroes `sums` (one launch: the
 * statistics pass for outputs whose producing GEMM could not leave them, e.g. split-K products). */
int pcrcg_instnorm_colsums(const float* x, int n, int c, int ldx, void* sums, void* stream);
int pcrcg_instnorm_apply_sums(const float* x, int n, int c, int ldx, const void* sums, double count, float eps,
                              const float* res, int ldr, const void* res_sums, float slope, float* y, int ldy,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * PCR-CG's image-feature injection (ref:models/architectures.py:195-514): the geometric input feature (a column of
 * ones) becomes [N, c+1] = ones, and every 3-D point that projects into a colour image receives that pixel's 2-D
 * feature in columns 0..c-1 (column c stays 1):
 *     x[inds3d[j] + row_offset, 0:c] = fmap[:, inds2d[j,1], inds2d[j,0]] * valid[inds2d[j,0], inds2d[j,1]]
 * fmap [c, h, w] f32 is the 2-D backbone's output for one image (the backbone itself is outside the path; any
 * producer of such a map plugs in), valid [w, h] f32 its valid-pixel mask as the reference stores it (NULL: none,
 * the three-image branch :196-252), inds2d [n, 2] i64 = (column, row), inds3d [n] i64 = point index inside its cloud,
 * row_offset = 0 for the source cloud / the source cloud's size for the target cloud (:239-241).  The reference
 * writes image 3, 2, 1 in that order so that image 1 wins where projections overlap: call once per image in the
 * same order on the same stream.  pcrcg_fill2d writes the constant (ones) matrix first.
 * ---------------------------------------------------------------------------------------------- */
int pcrcg_fill2d(float* dst, int ld, int rows, int cols, float value, void* stream);
int pcrcg_inject_image_features(const float* fmap, int c, int h, int w, const float* valid, const int64_t* inds2d,
                                const int64_t* inds3d, int n, long row_offset, long n_rows, float* x, int ldx,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * The projections and valid maps themselves, computed on the device from raw frames (the reference computes them on
 * the CPU in its data loader, ref:datasets/indoor.py:284-299,587-616).
 *
 * pcrcg_project_depth: Projection.projection(points, depth_map, world2camera) (ref:projection.py) for one cloud and one
 *   depth map.  points [n, 3] f32, depth [h, w] f32; h_world2camera and h_intrinsics are 16 row-major floats in HOST
 *   memory (a 3x3 intrinsic matrix is embedded in the identity first, as the reference does).  Writes inds2d [k, 2] i64
 *   (column, row) and inds3d [k] i64 (ascending point index, as the reference's boolean masks leave it), k <= n, and the
 *   count k as one int32 on the device -- no host round trip.  Point p is kept iff, with (u, v, z) = K [W p; 1] rounded
 *   like the reference's two CPU torch.mm calls (the k-ordered fused chain fma(m3, 1, fma(m2, p2, fma(m1, p1, m0 p0)))),
 *   u / z and v / z (IEEE division) lie in (-1, w) and (-1, h) -- .long() truncates toward zero -- and
 *   |z - depth[trunc(v/z), trunc(u/z)]| < thresh.  Points at or behind the camera are not rejected (the reference does
 *   not either).  Workspace: pcrcg_project_depth_ws_bytes(n).
 *
 * pcrcg_inject_frames: the fused form of pcrcg_fill2d + pcrcg_project_depth + pcrcg_inject_image_features for one pair:
 *   x [n_points, ldx] (rows of the source cloud then the target cloud, len_src of them source) gets, per point, the
 *   features of the LAST frame of its side (frames in the reference's write order, as for pcrcg_inject_image_features)
 *   whose projection keeps it: columns 0..c-1 = fmap[:, row, column] * valid[column, row], column c = 1, columns
 *   c+1..ldx-1 = 0; a point no frame keeps gets ones in columns 0..c and zeros after.  Every row is written once, bit for
 *   bit what the unfused sequence writes.  h_frames: n_frames <= 6 host structs, at most 3 per side; fmap [c, h, w] and
 *   depth [depth_h, depth_w] must have the same size.  One launch; nothing is allocated or synchronised.
 *
 * pcrcg_superglue_valid_maps: the two valid maps of one image pair from SuperGlue's output (ref:datasets/indoor.py:
 *   284-299): keypoints0 [n0, 2], keypoints1 [n1, 2] f32 (x, y), matches [n0] i64 (-1: unmatched), confidence [n0] f32.
 *   src_valid / tgt_valid [map_w, map_h] f32 (the reference's [160, 120]: first index the column x) = 0, then for every
 *   valid match i in order map[int(kx - window) : int(kx + window), int(ky - window) : int(ky + window)] = confidence[i]
 *   with (kx, ky) = keypoints0[i] (source) and keypoints1[matches[i]] (target); int() of the exact value, the bounds under
 *   numpy's slice rules (negative counts from the end, then clamps at 0; past the end clamps; start >= stop paints
 *   nothing).  A match with matches[i] >= n1 or a non-finite keypoint (either of its two) paints nothing, on either map.
 *
 * Bad arguments (null pointers, sizes <= 0, h * w >= 2^31, ldx < c + 1, more than 3 frames of a side, a depth / fmap
 * size mismatch) are rejected with PCRCG_EBADARG before anything launches.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pcrcg_image_frame {
    const float* fmap;      /* [c, h, w] f32: the 2-D backbone's output for this image */
    const float* depth;     /* [depth_h, depth_w] f32 */
    const float* valid;     /* [w, h] f32 or NULL (no valid map) */
    float world2camera[16]; /* row-major, by value */
    float intrinsics[16];   /* row-major, by value */
    float thresh;           /* depth test bound (Projection's thresh, 0.1) */
    int h, w;               /* fmap's size */
    int depth_h, depth_w;   /* must equal h, w */
    int target;             /* 0: the frame of the source cloud, 1: of the target cloud */
} pcrcg_image_frame;

size_t pcrcg_project_depth_ws_bytes(int n);
int pcrcg_project_depth(const float* points, int n, const float* depth, int h, int w, const float* h_world2camera,
                        const float* h_intrinsics, float thresh, int64_t* inds2d, int64_t* inds3d, int* k, void* ws,
                        size_t ws_bytes, void* stream);
int pcrcg_inject_frames(const float* points, long n_points, long len_src, const pcrcg_image_frame* h_frames, int n_frames,
                        int c, float* x, int ldx, void* stream);
int pcrcg_superglue_valid_maps(const float* keypoints0, int n0, const float* keypoints1, int n1, const int64_t* matches,
                               const float* confidence, int window, int map_w, int map_h, float* src_valid, float* tgt_valid,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * GNN head helpers (ref:models/gcn.py).  Non-finite feature values: the rule under "Point-wise blocks" (emax is a
 * NaN-propagating maximum; kNN selection on non-finite coordinates is undefined).
 * ---------------------------------------------------------------------------------------------- */
/* get_graph_feature's kNN (ref:models/gcn.py:15-34,48-51): dist = -2ab + a^2 + b^2 clamped at 1e-12,
 * each step rounded as the reference's CPU run rounds it; the k+1 smallest, first dropped.  Among exactly equal
 * distances the order -- and which of them survive the cut -- is that of torch.topk's CPU kernel for k <= 10
 * (its std::partial_sort / std::nth_element + std::sort, replayed), and plain (dist, index) order for k > 10.
 * coords [n,3] f32 -> idx [n,k] i32. */
int pcrcg_knn(const float* coords, int n, int k, int* idx, void* stream);
/* DGCNN edge conv after splitting the 1x1 conv over cat(f_i, f_j - f_i) into a centre term and a
 * neighbour term (ref:models/gcn.py:61-62,123-129):  e[i,j,c] = ctr[i,c] + nbr[idx[i,j],c];
 *   emax[i,c] = max_j e[i,j,c];  stats[2*c] = (mean, rstd) of e over all (i,j) (InstanceNorm2d).
 * The caller finishes with pcrcg_instnorm_apply(emax, stats, slope 0.2) -- max commutes with the
 * monotone normalise + LeakyReLU.  ctr/nbr/emax row-major [n,c] with leading dims. */
size_t pcrcg_edgeconv_ws_bytes(int c);
int pcrcg_edgeconv_reduce(const float* ctr, int ld_ctr, const float* nbr, int ld_nbr, const int* idx,
                          int n, int k, int c, float eps, float* emax, int ld_emax, float* stats,
                          void* ws, size_t ws_bytes, void* stream);
/* The same reduction leaving the statistics as fp64 sums: sums [2][c] f64 (zeroed by the caller) += (sum, sum of squares)
 * of e over all (i,j); finish with pcrcg_instnorm_apply_sums(emax, ..., sums, count = n * k, ...).  One launch. */
int pcrcg_edgeconv_reduce_sums(const float* ctr, int ld_ctr, const float* nbr, int ld_nbr, const int* idx, int n, int k,
                               int c, float* emax, int ld_emax, void* sums, void* stream);
/* Row softmax in place: x [rows, cols] (ld), x = softmax(x * scale) (ref:models/gcn.py:151-155,
 * ref:models/architectures.py:562-563). */
int pcrcg_softmax_rows(float* x, int rows, int cols, int ld, float scale, void* stream);
/* Multi-head attention in ONE launch (ref:models/gcn.py:151-155: scores = q k^T / sqrt(d), prob = softmax(scores),
 * message = prob v, per head):  out[:, h*d:(h+1)*d] = softmax(scale * q_h k_h^T) v_h  for h < heads, where head h of
 * q [n, heads*d], k / v [ms, heads*d] and out [n, heads*d] is the column block [h*d, (h+1)*d) (row-major, leading
 * dimensions ldq/ldk/ldv multiples of 4, 16-byte aligned bases).  d in {16, 32, 48, 64, 128}
 * (pcrcg_attention_supported); other widths: one pcrcg_gemm_f32 / pcrcg_softmax_rows / pcrcg_gemm_f32 per head. */
int pcrcg_attention_supported(int d);
int pcrcg_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* out, int ldo, int n,
                    int ms, int heads, int d, float scale, void* stream);
/* y[r * ldy] = sum_j softmax(scale * x[r, :])_j * vec[j * ldv]: the saliency scores
 * (ref:models/architectures.py:562-563, softmax(inner / T) @ scores) without storing the probabilities. */
int pcrcg_softmax_matvec(const float* x, int rows, int cols, int ld, float scale, const float* vec, int ldv, float* y,
                         int ldy, void* stream);

/* Copy a device status word to the host after draining `stream`; returns PCRCG_ECAPACITY if it is
 * non-zero. */
int pcrcg_check_status(const int* status, void* stream);

/* Small element-wise helpers used by the network runner (also exported for tests).
 *   copy2d : dst[r, 0:cols] = src[r, 0:cols]                       (torch.cat pieces)
 *   add    : dst = a + b                                          (residual of ref:models/gcn.py:213-214)
 *   l2norm : dst[r,:] = src[r,:] / max(|src[r,:]|, 1e-12)          (F.normalize, ref:architectures.py:541,582)
 *   scores : dst[r] = scrub(clamp(sigmoid(src[r*ld]), 0, 1))      (ref:architectures.py:176-179,576-579) */
int pcrcg_copy2d(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols, void* stream);
int pcrcg_add(const float* a, const float* b, float* dst, long n, void* stream);
int pcrcg_l2norm_rows(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols, void* stream);
int pcrcg_sigmoid_scores(const float* src, int ld_src, float* dst, int rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-network runner: KPFCNN.forward (ref:models/architectures.py:181-191, 516-610) enqueued by ONE
 * call, so that the host cost per pair is a single FFI crossing instead of several hundred.
 * The descriptors are plain C structs of device pointers and sizes; pcrcg_amd/runner.py builds them
 * from the nn.Module tree (weights as stored in the reference state_dict, plus a few re-packed copies
 * noted below).
 * ---------------------------------------------------------------------------------------------- */
#define PCRCG_MAX_LEVELS 8
#define PCRCG_MAX_BLOCKS 32
#define PCRCG_MAX_GNN 8

enum { PCRCG_BLK_SIMPLE = 0, PCRCG_BLK_RESNETB = 1, PCRCG_BLK_UNARY = 2, PCRCG_BLK_LAST_UNARY = 3,
       PCRCG_BLK_UPSAMPLE = 4 };

typedef struct pcrcg_block {
    int type;            /* PCRCG_BLK_* */
    int layer;           /* layer_ind of the reference block */
    int strided;         /* queries = level layer+1, table = pools[layer] */
    int in_dim, out_dim; /* feature widths seen by the block (out_dim = produced width) */
    int mid_dim;         /* KPConv width of a resnetb block (out_dim/4); KPConv output of a simple block */
    float extent;        /* KP_extent of the block's KPConv */
    const float* kp;     /* [15,3]  ...KPConv.kernel_points */
    const float* kp_w;   /* [15*cin, cout]  ...KPConv.weights */
    const float* kp_wt;  /* [cout, 15*cin]  K-contiguous copy: the contraction then is a C = A * B^T product, or NULL.
                            cin = 1: [cout, 16], the 16th column zero (the gather kernel then writes rows of 16 floats) */
    const float* kp_w_pad; /* [15*cin_pad, cout]: kp_w with the input channels zero-padded to cin_pad (a multiple of
                              4), or NULL.  Set when cin % 4 != 0 (PCR-CG's 129-channel first layer,
                              ref:models/architectures.py:195-514): the runner pads the features likewise, so the
                              MFMA gather kernel applies instead of the scalar fallback. */
    int cin_pad;
    const float* unary1; /* [mid, in] or NULL (nn.Identity) */
    const float* unary2; /* [out, mid] */
    const float* shortcut; /* [out, in] or NULL (nn.Identity) */
    const float* mlp;    /* unary / last_unary: [out, in] with leading dimension mlp_ld (rows 16-B aligned) */
    int mlp_ld;
    const float* mlp_skip; /* unary / last_unary that consumes cat([upsampled x, skip]) (model.dec_concat): a dense,
                              16-byte aligned copy of the weight's skip columns [out, skip_dim] (= mlp[:, in - skip_dim:]),
                              or NULL.  With it the runner never materialises the upsampled matrix or the concatenation:
                              it runs mlp[:, :in - skip_dim] on rows gathered through the upsample table and adds the
                              skip part's product (ref:models/blocks.py:77-87, ref:models/architectures.py:568-569). */
    int mlp_skip_ld, skip_dim;
} pcrcg_block;

typedef struct pcrcg_gnn_layer {
    int cross;             /* 0 = SelfAttention (ref:models/gcn.py:96-134), 1 = AttentionalPropagation (:176-185) */
    /* self: 1x1 conv weights [cout, 2*cin] = [Wa | Wb] re-packed as [2*cout, cin] = [Wa-Wb ; Wb] (rows: the centre
     * term's output channels, then the neighbour term's), k-contiguous like every other weight */
    const float* edge1;    /* [2c, c] */
    const float* edge2;    /* [4c, c] */
    const float* conv3;    /* [c, 4c] as stored ([out, in]) */
    /* cross: projection weights with output channels permuted head-major, [c, c] as [out, in] */
    const float *wq, *bq, *wk, *bk, *wv, *bv;
    const float *wm, *bm;  /* merge, input channels permuted head-major */
    const float *w0, *b0;  /* mlp.0 [2c, 2c] */
    const float *w3, *b3;  /* mlp.3 [c, 2c] */
} pcrcg_gnn_layer;

typedef struct pcrcg_model {
    int n_enc, n_dec, n_gnn;
    pcrcg_block enc[PCRCG_MAX_BLOCKS];
    pcrcg_block dec[PCRCG_MAX_BLOCKS];
    pcrcg_gnn_layer gnn[PCRCG_MAX_GNN];
    int enc_skip[PCRCG_MAX_BLOCKS];   /* 1 if the input of encoder block i is saved as a skip (:521-522) */
    int dec_concat[PCRCG_MAX_BLOCKS]; /* 1 if decoder block i consumes cat([x, skip]) (:568-569) */
    int enc_out_dim, gnn_dim, heads, knn_k, final_dim;
    const float *bottle_w, *bottle_b;         /* [gnn, enc_out], [gnn] */
    const float *proj_gnn_w, *proj_gnn_b;     /* [gnn, gnn], [gnn] */
    const float *proj_score_w, *proj_score_b; /* [1, gnn], [1] */
    float temperature;                        /* exp(epsilon) + 0.03 (:561) */
    int feature_bf16;                         /* 0: fp32 feature storage (the parity-tested path, default).  1: the
                                                 bf16 feature-storage VARIANT (BASELINE.json configs[1] "bf16/fp32"):
                                                 inside every KPConv with cin % 32 == 0 the neighbour gathers read a
                                                 bf16 copy of the features and the aggregated [nq, 15*cin] matrix is
                                                 bf16 in HBM; weights, accumulation, norms, outputs stay fp32.  NOT
                                                 within the 1e-4 parity bound: tests/test_bf16_gpu.py states its error */
} pcrcg_model;

typedef struct pcrcg_table { const int64_t* idx; int rows, cols, ld; } pcrcg_table;

typedef struct pcrcg_batch {
    int n_levels;
    const float* points[PCRCG_MAX_LEVELS];
    int n_points[PCRCG_MAX_LEVELS];
    pcrcg_table neighbors[PCRCG_MAX_LEVELS], pools[PCRCG_MAX_LEVELS], upsamples[PCRCG_MAX_LEVELS];
    const float* features; /* [n_points[0], feat_dim]; feat_dim = the first block's in_dim, or its cin_pad when it carries
                              kp_w_pad (features handed over already zero-padded); anything else is PCRCG_EBADARG */
    int feat_dim;
    int len_src_c;         /* stack_lengths[-1][0] */
    const int* stack_lengths[PCRCG_MAX_LEVELS]; /* [nb] i32 per level (device); filled by pcrcg_pyramid_build,
                                                   not read by pcrcg_kpfcnn_forward (may be NULL) */
} pcrcg_batch;

typedef struct pcrcg_outputs {
    float* feats_f;         /* [n0, final_dim] */
    float* scores_overlap;  /* [n0] */
    float* scores_saliency; /* [n0] */
} pcrcg_outputs;

size_t pcrcg_kpfcnn_ws_bytes(const pcrcg_model* model, const pcrcg_batch* batch);
int pcrcg_kpfcnn_forward(const pcrcg_model* model, const pcrcg_batch* batch, const pcrcg_outputs* out, void* ws,
                         size_t ws_bytes, void* stream);

/* The same forward for n (1 to 4) INDEPENDENT fragment pairs in one call: batches[n], outs[n] (e.g. the batches one
 * pcrcg_pyramid_build call with cfg.group = 2 returns for 2n clouds).  Pairs never mix -- InstanceNorm statistics, neighbour tables,
 * the GNN's kNN and attention stay per pair (ref:datasets/dataloader.py:207 asserts one pair per batch;
 * ref:models/blocks.py:456-463 normalises over the batch's stacked points), so the outputs are those of n separate
 * pcrcg_kpfcnn_forward calls up to fp32 summation order -- but every product with a weight matrix runs ONCE for all
 * pairs (their row ranges sharing the weight operand in one launch): the coarse-level products, which fill a fraction of
 * the chip for one pair, fill twice that at the same duration, and a pair costs half the GEMM launches.
 * Per-pair kernels (gathers, normalisation, kNN, attention) are enqueued once per pair.  With the fp32-MFMA arithmetic
 * (pcrcg_gemm_set_mode(0)) the products run pair by pair as well. */
size_t pcrcg_kpfcnn_group_ws_bytes(const pcrcg_model* model, const pcrcg_batch* batches, int n);
int pcrcg_kpfcnn_forward_group(const pcrcg_model* model, const pcrcg_batch* batches, const pcrcg_outputs* outs, int n,
                               void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pyramid builder: the whole front end of one fragment pair behind one call -- the pyramid loop of
 * collate_fn_descriptor (ref:datasets/dataloader.py:230-361: per level a conv table, then grid subsampling, a pool
 * and an upsample table; radius and cell size double per level) with batch_grid_subsampling_kpconv /
 * batch_neighbors_kpconv (:14-69) underneath.  It sequences the front-end entry points above over one arena and
 * fills the pcrcg_batch that pcrcg_kpfcnn_forward consumes; every pointer in `out` points into `ws`.
 *   cfg        level plan: r_conv / r_pool / dl per level (ref:datasets/dataloader.py:239,286,301,357), has_conv,
 *              pooled (every level but the last), limit = neighborhood_limits; tie_order 0 = ascending index inside
 *              groups of exactly equal distance, 1 = the reference's order (rows holding such groups are redone
 *              through the KD-forest, as pcrcg_radius_reorder_jobs documents).
 *   out        one pcrcg_batch (cfg->group == 0) or nb / cfg->group of them
 *   ws         arena of pcrcg_pyramid_ws_bytes(n0, nb, cfg) bytes.  cfg->shrink in (0,1] is the caller's bound on
 *              rows(level l+1) / rows(level l) (1.0 = always enough; 3DMatch-like clouds keep about a quarter): level l is
 *              given room for n0 * shrink^l rows, and since round 6 that bound -- not a row count read back from the GPU --
 *              sizes every buffer, table and launch of the level.  A cloud that keeps more rows than the bound allows is
 *              reported as PCRCG_EWORKSPACE at the end of the call -- nothing is corrupted, call again with a larger
 *              shrink (and the arena that goes with it).
 *   h_scratch  HOST scratch of >= 256 ints, pinned for best latency: the call uses 2 + 3 n_levels (P + 2) + n_levels
 *              + n_levels nb of them (P = nb / group, or 1), at most 254 under the argument checks (n_levels <= 4,
 *              P <= 14, n_levels nb <= 64), and rejects anything above 256; h_lengths HOST [n_levels * nb] receives the
 *              per-level cloud lengths (stack_lengths); h_status HOST int (pinned; may be NULL) receives the tie-order
 *              restore status word ASYNCHRONOUSLY -- valid once `stream` has drained, 0 = fine, else as documented at
 *              pcrcg_radius_reorder_jobs.
 *   deferred   NULL: the tie-order restore step (KD-forest + reorder of the rows holding ties) is enqueued on `stream`
 *              by this call.  Otherwise the call only DESCRIBES it in *deferred (pointers into `ws`) and the caller
 *              enqueues it with pcrcg_pyramid_restore_run on a stream of its choice that is ordered after `stream`'s
 *              work and before the first reader of the tables (the pair engine runs it on the pair's model stream:
 *              the front-end stream is the pipeline's bottleneck).
 * The call WAITS for `stream` ONCE, at the end of the kernel chain, for the row counts of the levels and the tables'
 * column counts (one copy of ~100 words): the levels are sized from cfg->shrink, every kernel takes its row count from
 * the cloud lengths on the device.  (Rounds 2-5 read every subsampled level's row count back before sizing the next:
 * four round trips per call, ~1.1 ms of idle front-end stream per four-pair chain.)  It holds no global state, so several
 * host threads may build pyramids on several streams concurrently.  The last launches (tie-order restore) are still in
 * flight when it returns.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pcrcg_pyramid_cfg {
    int n_levels;
    float r_conv[PCRCG_MAX_LEVELS], r_pool[PCRCG_MAX_LEVELS], dl[PCRCG_MAX_LEVELS];
    int has_conv[PCRCG_MAX_LEVELS], pooled[PCRCG_MAX_LEVELS], limit[PCRCG_MAX_LEVELS];
    int tie_order;
    int group;   /* 0: all nb clouds form ONE batch (the reference's contract).  g > 0: the clouds are nb / g independent
                    groups of g clouds (g = 2: several fragment pairs stacked into one call); `out` then is an array of
                    nb / g batches, each with its own tables (indices relative to the group's supports, the group's own
                    column counts) -- what nb / g separate calls would have produced, from ONE chain of kernels: the
                    chain is latency-bound, so two pairs cost little more than one */
    int up_nearest; /* 0: upsample tables with `limit` columns, as collate_fn_descriptor builds them
                       (ref:datasets/dataloader.py:287-297).  1: ONE column -- the nearest coarse point within the radius
                       (the reference's order among equidistant ones), which is all that the network reads of them
                       (closest_pool, ref:models/blocks.py:77-87): for hosts that feed pcrcg_kpfcnn_forward and nothing
                       else, the search keeps one candidate per row instead of sorting and writing `limit` of them */
    double shrink;  /* bound on rows(level l+1) / rows(level l), in (0,1]; 0 or out of range = 1.0 (see `ws` above) */
    void* side_stream;  /* NULL, or further streams (hipStream_t) of the caller's: the chain is a DAG -- a level's subsampling  */
    void* side_stream2; /* needs only the level's points, as do its cell grid and conv search; a KD-forest of the restore step
                       needs only its levels' points.  side_stream: the subsamplings run there, back to back from the moment
                       the input is in place, beside the grids and searches on `stream`, which waits for each subsampled
                       level when it first reads it.  side_stream2: the KD-forests (tie_order = 1) -- level 0's at once, the
                       subsampled levels' when the last of them exists; NULL: behind the subsamplings on side_stream.
                       `stream` waits for all of it before the call returns.  Both NULL: one stream, one line of kernels.
                       Which streams: gfx950 has four hardware dispatchers and a dispatcher hands out one kernel's workgroups at
                       a time (pcrcg_stream_pipe_classes).  Side streams on OTHER dispatchers than `stream`'s -- idle ones --
                       halve the chain (one 2 x 30 000-point pair 1.01 against 1.65 ms, four pairs 1.85 against 3.17:
                       profiles/r06_chain_latency_alone.txt); side streams on `stream`'s own dispatcher gain nothing; side
                       streams on a dispatcher that also serves a stream of large kernels stand behind every one of those
                       (the pair engine, whose other three dispatchers run the forwards, builds its chains in line). */
} pcrcg_pyramid_cfg;
typedef struct pcrcg_pyramid_restore {
    int njobs;                                   /* 0: no row holds a tie, nothing to do but post the status word */
    pcrcg_reorder_job jobs[PCRCG_MAX_REORDER_JOBS]; /* every job names its forest (sup / forest / forest_ns / forest_nb): the
                                                    builder keeps two, level 0's and one over the subsampled levels, and has
                                                    enqueued their builds -- they exist once `stream`'s work has passed */
    int* tie_status;                             /* device status word */
} pcrcg_pyramid_restore;
/* Threads: calls from several host threads are independent (arena, h_scratch and outputs are the caller's).  Calls that name
 * the SAME stream hold that stream's enqueue lock while they enqueue their chain and release it before they wait for their
 * round trip: the chains stay whole, one behind the other, and one call's wait overlaps the next call's enqueue (with
 * `deferred` set nothing of a call is left in the stream when it returns; without it the restore step follows whatever
 * another thread has enqueued meanwhile).  profiles/r06_ab_overlapped_builds.txt. */
size_t pcrcg_pyramid_ws_bytes(int n0, int nb, const pcrcg_pyramid_cfg* cfg);
int pcrcg_pyramid_build(const float* pts, int n0, const int* len, int nb, const pcrcg_pyramid_cfg* cfg, void* ws,
                        size_t ws_bytes, int* h_scratch, pcrcg_batch* out, int* h_lengths, int* h_status,
                        pcrcg_pyramid_restore* deferred, void* stream);
/* The same build with the input clouds given in `parts` pieces (e.g. the two pairs of a cfg.group = 2 build, each where
 * its producer left it): part i has n_parts[i] rows at pts_parts[i] and nb_parts[i] cloud lengths at len_parts[i] (device);
 * the builder copies them behind each other into its arena -- it copies its input anyway -- so the caller runs no
 * concatenation kernel.  Row for row the result of pcrcg_pyramid_build on the concatenated input. */
int pcrcg_pyramid_build_parts(const float* const* pts_parts, const int* n_parts, const int* const* len_parts,
                              const int* nb_parts, int parts, const pcrcg_pyramid_cfg* cfg, void* ws, size_t ws_bytes,
                              int* h_scratch, pcrcg_batch* out, int* h_lengths, int* h_status,
                              pcrcg_pyramid_restore* deferred, void* stream);
int pcrcg_pyramid_restore_run(const pcrcg_pyramid_restore* r, int* h_status, void* stream);

/* A non-blocking HIP stream created by the library (hipStreamCreateWithPriority(hipStreamNonBlocking); priority 0 =
 * default, -1 = high) for hosts that have no stream abstraction of their own; *stream receives a hipStream_t. */
int pcrcg_stream_create(void** stream, int priority);
int pcrcg_stream_destroy(void* stream);
/* Which of the caller's n (<= 64) streams share a hardware dispatcher.  gfx950's command processor has four compute
 * dispatchers; every stream's hardware queue belongs to one of them, and a dispatcher hands out the workgroups of one kernel
 * at a time -- two busy streams on the same dispatcher take turns, kernel by kernel, instead of running side by side
 * (profiles/r06_queue_pipes.txt).  cls[i] receives the class of streams[i] (0 = streams[0]'s class, then 1, 2, .. by first
 * appearance).  The classes are MEASURED (~1.5 ms per test on an idle GPU: a dispatch-bound probe kernel on one stream, a
 * one-workgroup kernel on the other); scratch = 16 bytes of device memory.  A host that runs several streams side by side
 * (pcrcg_amd/pairstream.py) picks them from different classes, and puts streams of small, latency-bound kernels that should
 * not wait for each other's resources -- the front-end chain and its KD-forests -- into one. */
int pcrcg_stream_pipe_classes(void* const* streams, int n, int* cls, void* scratch);

/* ------------------------------------------------------------------------------------------------
 * Registration back end
 * Replaces ransac_pose_estimation (ref:lib/benchmark_utils.py:187-224): open3d 0.10's
 * registration_ransac_based_on_feature_matching (mutual = False) and _based_on_correspondence on the mutual pairs of the
 * inner-product score (mutual = True).  open3d seeds its RANSAC per OpenMP thread, so this is a deterministic algorithm of
 * the same structure rather than a bit-for-bit copy; DESIGN.md section 10 defines it and tests/ransac_ref.py restates it.
 *
 * pcrcg_feature_match: the correspondence list corr [k_max, 2] int32 = (source index, target index) and its length k (ONE
 * device int) for source / target descriptors [n, c] / [m, c] (row strides ld_src, ld_tgt >= c).
 *   mutual = 0: row i = (i, nn(i)), nn(i) = the target nearest in L2 feature distance (the arg-max of <a_i, b_j> - |b_j|^2/2
 *               in fp32, lowest index on ties); k = n, so k_max = n.
 *   mutual = 1: the pairs (i, j) with j = argmax_j <a_i, b_j> and i = argmax_i <a_i, b_j> (first index on ties), in
 *               ascending source index; k <= min(n, m), give k_max = n.
 * pcrcg_ransac: src [n, 3], tgt [m, 3] f32 points; grid = pcrcg_cellgrid_build over the m target points as ONE cloud with
 * radius = (float)threshold; corr / k as above (k is clamped to k_max).  With P = k:
 *   hypothesis h < max_iteration draws rows ((r >> 32) * P) >> 32, r = splitmix64((seed << 40) + 8 h + s), s < ransac_n,
 *     splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *     return z ^ z >> 31   (all mod 2^64; seed < 2^24);
 *   and passes iff, in this order: its source ids are distinct; (edge_similarity > 0) every pair of samples has float64
 *   edge lengths ds, dt with ds >= dt * sim and dt >= ds * sim; the float64 Kabsch fit without scaling (reflection fixed by
 *   diag(1, 1, det)) has sigma_2 > 1e-12 sigma_1 of the 3 x 3 cross-covariance; (distance_check) |T p_s - p_t| <= threshold
 *   for every sample, in float64.
 *   The first max_validation passing hypotheses are evaluated: R|t rounded to fp32, every source point moved with unfused
 *   fp32 arithmetic ((r0 x + r1 y) + r2 z) + t0, its nearest target point within the threshold looked up; an inlier iff
 *   d2 < (float)(threshold^2), d2 = ((dx dx + dy dy) + dz dz) in fp32; count = inliers, sum = float64 sum of their d2.
 *   The best has the highest count, then the lowest sum, then the lowest h.
 *   out_transform [16] f64 (row-major 4 x 4) = its float64 fit, not refined; identity when no hypothesis passes or none
 *   has an inlier.  out_stats [6] f64 = (fitness = count / n, inlier_rmse = sqrt(sum / count), k, iterations = max_iteration,
 *   validations, chosen h or -1); fitness and rmse are 0 for the identity.
 *   pcrcg_ransac does not read the grid's overflow flag: a target point with a coordinate beyond 2^20 cells of the
 *   threshold is never found by the evaluation (no source point counts as its inlier), a moved source point beyond that
 *   range is no inlier either, every other point is counted as usual, and nothing is reported.
 * trace (NULL, or any member NULL: not written) receives the stages for tests:
 *   samples [max_iteration, ransac_n] i32 rows drawn, pass [max_iteration] i32, xf32 / xf64 [max_iteration, 12] the fit as
 *   R (row-major) then t (zero where a check before the fit failed), valid_ids [max_validation] i32, counts
 *   [max_validation] i32, sums [max_validation] f64 (the first `validations` entries are written).
 * Both entries take a workspace of pcrcg_ransac_ws_bytes(n, m, max_iteration, max_validation) bytes (one size serves both,
 * reused on the same stream), allocate nothing and synchronise nothing.  Bad arguments (null pointers, ransac_n outside
 * 3..8, k_max < ransac_n, max_validation > max_iteration, threshold <= 0, edge_similarity outside [0, 1]) are rejected
 * before anything launches.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pcrcg_ransac_trace {
    int* samples;
    int* pass;
    float* xf32;
    double* xf64;
    int* valid_ids;
    int* counts;
    double* sums;
} pcrcg_ransac_trace;

size_t pcrcg_ransac_ws_bytes(int n, int m, int max_iteration, int max_validation);
int pcrcg_feature_match(const float* src_feat, int ld_src, int n, const float* tgt_feat, int ld_tgt, int m, int c, int mutual,
                        int* corr, int* k, void* ws, size_t ws_bytes, void* stream);
int pcrcg_ransac(const float* src, int n, const float* tgt, int m, const void* grid, const int* corr, int k_max, const int* k,
                 int ransac_n, double threshold, double edge_similarity, int distance_check, int max_iteration,
                 int max_validation, uint64_t seed, double* out_transform, double* out_stats, const pcrcg_ransac_trace* trace,
                 void* ws, size_t ws_bytes, void* stream);

/* Several pairs per call: B independent pairs in one set of launches.  Pair b's result is exactly (bit for bit: transform,
 * statistics) that of pcrcg_feature_match with mutual = 0 followed by pcrcg_ransac on that pair alone with seed = seeds[b];
 * no pair affects another, and nothing depends on the order of the pairs or on B (no floating-point atomics).
 * Mutual correspondences are not offered by these two entries (every reference tester uses mutual = False); the batched
 * mutual L2 list is pcrcg_mutual_match_batch ("Fast global registration" below).
 *   Layout: the pairs are ragged and concatenated.  src [n_total, 3], tgt [m_total, 3] f32; src_off / tgt_off [B + 1] i32
 *   DEVICE arrays of row offsets (src_off[0] = 0, non-decreasing, src_off[B] = n_total; likewise tgt_off); descriptors
 *   [n_total, c] / [m_total, c] with row strides ld_src / ld_tgt.  corr [n_total, 2] i32: pair b's rows start at
 *   src_off[b] and hold indices local to the pair; k [B] i32 its list lengths (= n_b).  seeds [B] u64 (DEVICE, each
 *   < 2^24), out_transform [B, 16] f64, out_stats [B, 6] f64 as pcrcg_ransac's, pair by pair.
 *   grid = pcrcg_cellgrid_build over the m_total concatenated targets with nb = B, slen = the pair lengths and
 *   radius = (float)threshold; pair b is looked up in its own hash table (the 2 m_b slots at 2 tgt_off[b]).
 *   n_max / m_max (host) must be >= every pair's source / target length; they only size the launch grids of
 *   pcrcg_feature_match_batch;
 *   pcrcg_ransac_batch needs m_total instead, because the grid's layout depends on it.  ransac_n, threshold, the checkers
 *   and the iteration and validation caps are the same for every pair of one call.
 *   The offsets and seeds live on the device and are not read by the host: a pair with n_b < ransac_n or m_b = 0 gets the
 *   identity (as when nothing passes), and a pair whose seed is >= 2^24 gets NaN in all of its 22 outputs.
 * Workspace: pcrcg_ransac_batch_ws_bytes(B, n_total, m_total, max_iteration, max_validation) bytes, one size for both
 * entries (reused on the same stream) = max(8 n_total + 4 m_total,
 *   8 B max_iteration + 64 B max_validation + scan(B max_iteration)) plus alignment padding, with scan(x) the device-wide
 *   scan's scratch -- about 0.47 MB per pair at 50 000 / 1 000.  Unlike pcrcg_ransac, the fp32 R|t is kept for the
 *   validated hypotheses only (re-fitted after the compaction), not for all of them.  B <= 65535 and
 *   B * max_iteration < 2^31; 0 is returned for arguments out of range.  Both entries allocate nothing and synchronise
 *   nothing; bad arguments (null pointers, B outside 1..65535, and every rule of the single-pair entries that the host can
 *   check) are rejected with PCRCG_EBADARG before anything launches. */
size_t pcrcg_ransac_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration, int max_validation);
int pcrcg_feature_match_batch(const float* src_feat, int ld_src, const int* src_off, int n_total, int n_max,
                              const float* tgt_feat, int ld_tgt, const int* tgt_off, int m_total, int m_max, int c, int B,
                              int* corr, int* k, void* ws, size_t ws_bytes, void* stream);
int pcrcg_ransac_batch(const float* src, const int* src_off, const float* tgt, const int* tgt_off, int m_total, const void* grid,
                       const int* corr, const int* k, int B, int ransac_n, double threshold, double edge_similarity,
                       int distance_check, int max_iteration, int max_validation, const uint64_t* seeds,
                       double* out_transform, double* out_stats, void* ws, size_t ws_bytes, void* stream);

/* ICP refinement: batched point-to-point ICP, the local pass after RANSAC's global one (csrc/icp.hip; added under ABI
 * version 4, which it does not change).  It restates open3d 0.10's RegistrationICP with
 * TransformationEstimationPointToPoint(false) -- what ref:datasets/kitti.py:105-121 refines its ground truth with -- as a
 * deterministic algorithm; no bit parity with open3d is claimed.  DESIGN.md section 10 defines it, tests/icp_ref.py
 * restates it in numpy.
 *   Layout as pcrcg_ransac_batch's: src [n_total, 3] f32, the B pairs concatenated; src_off / tgt_off [B + 1] i32 DEVICE row
 *   offsets; grid = pcrcg_cellgrid_build over the m_total concatenated targets with nb = B, slen = the pair lengths and
 *   radius = (float)max_correspondence_distance (the grid holds the target points: they are not passed again).  n_max
 *   (host) >= every pair's source length sizes the launch grid.  init [B, 16] f64 DEVICE, row-major T_0 per pair, or NULL:
 *   the identity.  The distance d, max_iteration and the two convergence bounds are shared by all pairs of a call.
 *   Evaluate(T): R|t rounded to fp32; every source point moved as RANSAC's evaluation moves it, ((r0 x + r1 y) + r2 z) + t0
 *     unfused; its nearest target among the 27 cells around it, d2 = ((dx dx + dy dy) + dz dz) in fp32, the LOWEST target
 *     index among equal d2; a correspondence iff d2 < (float)(d * d).  count = correspondences, sum = float64 sum of their
 *     d2; fitness = count / n_b, rmse = sqrt(sum / count) (0 when count = 0).
 *   Update: over the correspondences, with p the moved source point (the float64 value of the fp32 result) and q its
 *     target: S_p = sum p, S_q = sum q, S_pq = sum p q^T in float64; cs = S_p / count, ct = S_q / count,
 *     H = S_pq - S_p ct^T (an entry no larger than 1e-12 (|S_pq| + |S_p ct|) is rounding residue and counts as 0, so rows
 *     that all found ONE target give H = 0); delta = the Kabsch fit of pcrcg_ransac from H, cs, ct (the same device function: reflection fixed,
 *     degenerate iff sigma_2 <= 1e-12 sigma_1); T <- delta T in float64.  Every sum is reduced in a fixed order (inside a
 *     wavefront by a shuffle tree, the eight wavefronts of a 512-row workgroup in order, the workgroups in order); there are
 *     no floating-point atomics, so a pair's bits depend on its points and T_0 alone, not on B, its position or the run.
 *   Loop: Evaluate(T_0); for k = 1 .. max_iteration: update, Evaluate(T_k), stop if |fitness_k - fitness_k-1| <
 *     relative_fitness and |rmse_k - rmse_k-1| < relative_rmse (absolute differences, as open3d's).  Before an update the
 *     pair stops, keeping T, if count < 3 or the fit is degenerate.
 *   out_transform [B, 16] f64 = the last T; out_stats [B, 4] f64 = (fitness, rmse, count, updates applied) of its
 *   evaluation.  A pair with n_b = 0 or m_b = 0 returns T_0, fitness 0, 0 iterations; a pair whose T_0 is not finite, or
 *   whose n_b exceeds n_max, gets NaN in all 20 outputs (and no other pair is affected).
 *   trace (NULL, or any member NULL: not written), for tests: transforms [B, max_iteration + 1, 16] f64 = T_k, counts
 *   [B, max_iteration + 1] i32 and sums [B, max_iteration + 1] f64 of Evaluate(T_k), corr [max_iteration + 1, n_total] i32 =
 *   the pair-local target index of every source row in Evaluate(T_k), or -1; entries past a pair's last evaluation are not
 *   written.
 *   All 2 (max_iteration + 1) + 1 launches are enqueued at once; a DEVICE `done` word per pair makes the workgroups of a
 *   finished pair return at once, and the host reads nothing.  The entry allocates nothing and synchronises nothing.
 *   Workspace: pcrcg_icp_batch_ws_bytes(B, n_total, m_total, max_iteration) = 152 B + 132 (n_total / 512 + B + 1) bytes plus
 *   alignment padding (today a function of B and n_total alone); 0 for B outside 1..65535, a negative size or
 *   max_iteration outside 1..65536.  Bad arguments (null pointers, those ranges, n_max > n_total, d <= 0, a negative or
 *   NaN bound) are rejected with PCRCG_EBADARG and a short workspace with PCRCG_EWORKSPACE before anything launches. */
typedef struct pcrcg_icp_trace {
    double* transforms;
    int* counts;
    double* sums;
    int* corr;
} pcrcg_icp_trace;

size_t pcrcg_icp_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration);
int pcrcg_icp_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                    const void* grid, const double* init, int B, double max_correspondence_distance, int max_iteration,
                    double relative_fitness, double relative_rmse, double* out_transform, double* out_stats,
                    const pcrcg_icp_trace* trace, void* ws, size_t ws_bytes, void* stream);

/* Normal estimation: surface normals of B ragged clouds in ONE launch (csrc/normals.hip; added under ABI version 4, which
 * it does not change) -- open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)), what
 * ref:datasets/visualize.py:154-155 calls, restated as a deterministic algorithm; no bit parity with open3d is claimed.
 * DESIGN.md section 10 defines it, tests/normals_ref.py restates it in numpy.
 *   Layout: pts [n_total, 3] f32, the B clouds concatenated; off [B + 1] i32 DEVICE row offsets, never read by the host;
 *   grid = pcrcg_cellgrid_build over the same points with nb = B, slen = the cloud lengths and radius = (float)radius.
 *   n_max (host) >= every cloud's length sizes the launch (rows of a longer cloud past n_max are not written).
 *   viewpoints [B, 3] f64 DEVICE, or NULL: the origin (the sensor of a KITTI scan).
 *   Outputs: normals [n_total, 3] f64; optional (NULL: not written), for tests: count [n_total] i32 and cov [n_total, 6] f64.
 *   Definition, per point p_i of a cloud:
 *     Neighbours: the cloud's own points with d2 < (float)radius * (float)radius, d2 = ((dx dx + dy dy) + dz dz) in fp32,
 *       unfused; p_i itself is one of them.  They are taken in ascending (d2, cloud-local index) order and cut to the
 *       first max_nn: the library's radius-query contract, and open3d's hybrid search.  count = the length after the cut.
 *     Moments: d_k = (double)q_k - (double)p_i, k = count: m = sum d_k / k, C = sum d_k d_k^T / k - m m^T, in float64; the
 *       sums are taken over the neighbours in their (d2, index) order by a 64-lane shuffle tree (lane j holds neighbour j,
 *       zero beyond count), so they are a function of the row alone.  No floating-point atomics.
 *       cov = (xx, xy, xz, yy, yz, zz) of C.
 *     Normal: the unit eigenvector of C's smallest eigenvalue, by a float64 cyclic Jacobi on the symmetric 3 x 3 matrix
 *       (csrc/smallsolve.h).  count < 3, or C identically zero or not finite, gives (0, 0, 1) -- as it stands: the sign
 *       rule is not applied to this fallback.
 *     Sign: flipped so that n . (v - p_i) >= 0 with v the cloud's viewpoint; if that product is exactly 0, so that the
 *       first non-zero component is positive.
 *   A point with a NaN coordinate, or beyond 2^20 cells of the radius, has no neighbours (count = 0).
 *   The entry allocates nothing, synchronises nothing and reads nothing back.  Null pts / off / grid / normals / ws, B
 *   outside 1..65535, radius <= 0 or NaN, max_nn outside 1..64 and n_max > n_total are rejected with PCRCG_EBADARG before
 *   any launch; a short workspace with PCRCG_EWORKSPACE.  Workspace: pcrcg_estimate_normals_ws_bytes(B, n_total) (256 bytes
 *   today: the neighbour lists live in LDS); 0 for B outside 1..65535 or a negative n_total. */
size_t pcrcg_estimate_normals_ws_bytes(int B, int n_total);
int pcrcg_estimate_normals_batch(const float* pts, const int* off, int n_total, int n_max, const void* grid, int B, double radius,
                                 int max_nn, const double* viewpoints, double* normals, int* count, double* cov, void* ws,
                                 size_t ws_bytes, void* stream);

/* FPFH descriptors: the 33-bin Fast Point Feature Histograms of B ragged clouds in TWO launches (csrc/fpfh.hip; added under
 * ABI version 4, which it does not change) -- open3d 0.10's ComputeFPFHFeature(KDTreeSearchParamHybrid(radius, max_nn)),
 * restated as a deterministic algorithm; no bit parity with open3d is claimed.  DESIGN.md section 21 defines it,
 * tests/fpfh_ref.py restates it in numpy.
 *   Layout: pts, off, n_max and grid as pcrcg_estimate_normals_batch (the grid is built at THIS radius).
 *   normals [n_total, 3] f64 DEVICE, required: pcrcg_estimate_normals_batch's output, or the caller's own.
 *   Outputs: fpfh [n_total, 33] f32, one row per point (the [N, C] layout pcrcg_feature_match takes); optional (NULL: not
 *   written), for tests: count [n_total] i32, hist [n_total, 33] u8 and fpfh64 [n_total, 33] f64.
 *   Definition, per point p_i of a cloud, independent of every other cloud in the call:
 *     Neighbours: exactly the list of "Normal estimation" above -- the cloud's own points with fp32 unfused
 *       d2 < (float)radius * (float)radius, in ascending (d2, cloud-local index) order, cut to the first max_nn; k_i is its
 *       length (count).  max_nn ranges over 1..128 here.  A point with a NaN coordinate or out of cell range has k_i = 0 and
 *       is in nobody's list.
 *     Entry 0 is skipped (open3d skips "the point itself"): it is the point itself unless a coincident point with a lower
 *       index precedes it, and then the point pairs with itself at entry 1, with d = 0.
 *     Pair feature of (p, n1) with an entry (q, n2), in float64 from the widened fp32 coordinates, every operation rounded
 *       separately, dot products as ((x + y) + z), cross products as a b - c d per component:
 *         dp = q - p; d = sqrt(dp . dp); if d == 0: f = (0, 0, 0).
 *         a1 = (n1 . dp) / d, a2 = (n2 . dp) / d.  Swap iff |a1| < |a2|: n1 and n2 are exchanged, dp = -dp, f2 = -a2;
 *         otherwise f2 = a1.  (open3d compares acos(|a1|) > acos(|a2|): the same test without acos's rounding.)
 *         v = dp x n1; vn = sqrt(v . v); if vn == 0: f = (0, 0, 0).  v = v / vn; w = n1 x v; f1 = v . n2;
 *         f0 = atan2(w . n2, n1 . n2).
 *     Bins: h0 = floor(11 (f0 + M_PI) / (2 M_PI)), h1 = floor(11 (f1 + 1.0) 0.5), h2 = floor(11 (f2 + 1.0) 0.5), each
 *       clamped to 0..10; the pair counts in bins h0, 11 + h1 and 22 + h2.  A pair whose f is not all finite (a non-finite
 *       normal) counts in no bin, and still counts in k_i.
 *     SPFH: integer counts c_i[33] (hist; a bin holds at most 127); SPFH_i[j] = (double)c_i[j] * (100.0 / (k_i - 1)), zero
 *       for k_i <= 1.  (open3d adds 100 / (k_i - 1) c times: a difference in rounding only.)
 *     FPFH: over the entries e = 1 .. k_i - 1 in order, with D = ((dx dx + dy dy) + dz dz) in float64 (not the fp32 ranking
 *       key): if D == 0 the entry is skipped, otherwise F[j] = F[j] + SPFH_q[j] / D.  S_g = F[11 g] + ... + F[11 g + 10] in
 *       ascending order; if S_g != 0, F[j] = F[j] * (100.0 / S_g).  fpfh64[j] = F[j] + SPFH_i[j]; fpfh = (float)fpfh64.
 *       A row with k_i <= 1 is all zero.
 *   A row's bits depend on its cloud's points and normals alone: not on B, the order of the clouds or scheduling.  The bins are
 *   counted by integer adds, and nothing is added by floating-point atomics.
 *   The entry allocates nothing, synchronises nothing and reads nothing back.  Null pts / off / grid / normals / fpfh / ws, B
 *   outside 1..65535, radius <= 0 or NaN, max_nn outside 1..128 and n_max > n_total are rejected with PCRCG_EBADARG before
 *   any launch; a short workspace with PCRCG_EWORKSPACE.  Workspace: pcrcg_fpfh_ws_bytes(B, n_total, max_nn) =
 *   (n_total + 1) (40 + 4 max_nn) bytes plus alignment padding -- the lists' lengths, the byte histograms (36 bytes a row)
 *   and the ordered neighbour lists the second launch reads; 0 for B outside 1..65535, a negative n_total or max_nn outside
 *   1..128. */
size_t pcrcg_fpfh_ws_bytes(int B, int n_total, int max_nn);
int pcrcg_fpfh_batch(const float* pts, const int* off, int n_total, int n_max, const void* grid, int B, double radius, int max_nn,
                     const double* normals, float* fpfh, int* count, unsigned char* hist, double* fpfh64, void* ws,
                     size_t ws_bytes, void* stream);

/* ICP refinement with a choice of estimator (csrc/icp.hip; added under ABI version 4, which it does not change).
 * Everything pcrcg_icp_batch takes, plus
 *   estimation: 0 = point-to-point -- every output is pcrcg_icp_batch's, bit for bit; 1 = point-to-plane, open3d's
 *     TransformationEstimationPointToPlane;
 *   tgt_normals [m_total, 3] f64 DEVICE, in the targets' row order (pcrcg_estimate_normals_batch's output); required
 *     for estimation = 1, not read for 0.
 * Point-to-plane differs from the definition above in the update alone.  Evaluate(T) is unchanged -- the same moved point,
 * nearest target, tie rule, count, fitness and Euclidean rmse -- and convergence is tested on those, as open3d's loop does.
 *   Update: over the correspondences, with p the moved source point (the float64 value of the fp32 result), q its target
 *     and n the target's normal: r = ((p - q) . n), J = [p x n, n] (6 entries); A = sum J J^T (the 21 entries of the upper
 *     triangle, row by row), b = -sum J r (6), in float64 and in the fixed order of the other sums (shuffle tree, the eight
 *     wavefronts in order, the workgroups in order).  A x = b is solved by LDL^T with diagonal pivoting in float64
 *     (csrc/smallsolve.h) in the one lane that runs the Kabsch fit of estimation 0.  The pair stops, keeping T, if
 *     count < 6 or a pivot is <= 1e-12 times the largest (the relative rule of the Kabsch fit's sigma_2 <= 1e-12 sigma_1): a
 *     planar set of correspondences is degenerate.  delta = Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5), open3d's
 *     TransformVector6dToMatrix4d; T <- delta T in float64.
 *   A and b are even in n (every term holds n twice), so the result does not depend on the normals' signs, bit for bit.
 *   A normal that is not finite makes the pair's system not finite: the pair stops as a degenerate one.
 *   Range: J takes the moved point about the ORIGIN, as open3d's does, so A's rotation block grows with |p|^2 and cond(A)
 *     with (distance from the origin / extent of the cloud)^2.  From some hundreds of extents out (a 1 m cloud: between
 *     300 m and 1000 m) the smallest pivot falls to 1e-12 of the largest, the rule above refuses the update of a pair
 *     that is not degenerate at all, and the call returns its start with iterations = 0 and the start's fitness.  Callers
 *     re-centre such clouds, as for estimation 0.  Measured on a 1 m, 1 200-point corner cloud moved s metres along every
 *     axis (DESIGN.md section 10 has the table; numpy float64 / device): s = 0: cond(A) 28, 3 / 3 updates, worst point
 *     1.0e-9 m after; 10: 8.4e5, 4 / 4, 6.0e-7 m; 100: 7.0e9, 5 / 5, 5.4e-6 m; 1000: 6.8e13, smallest pivot 3.5e-14 of the
 *     largest, refused by both.
 *   Outputs, the NaN rules, empty pairs, the `done` word and the launch count are pcrcg_icp_batch's.
 *   trace: pcrcg_icp_trace's members, plus sums27 [B, max_iteration + 1, 27] f64 = A's upper triangle then b of
 *   Evaluate(T_k) (written for estimation = 1 only).
 *   Workspace: pcrcg_icp_batch_ex_ws_bytes(B, n_total, m_total, max_iteration) = 152 B + 228 (n_total / 512 + B + 1) bytes
 *   plus alignment padding, enough for either estimator; 0 as pcrcg_icp_batch_ws_bytes.  Bad arguments (pcrcg_icp_batch's,
 *   an estimation other than 0 or 1, estimation = 1 without normals) give PCRCG_EBADARG, a short workspace
 *   PCRCG_EWORKSPACE, before anything launches. */
typedef struct pcrcg_icp_trace_ex {
    double* transforms;
    int* counts;
    double* sums;
    int* corr;
    double* sums27;
} pcrcg_icp_trace_ex;

size_t pcrcg_icp_batch_ex_ws_bytes(int B, int n_total, int m_total, int max_iteration);
int pcrcg_icp_batch_ex(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                       const void* grid, const double* init, int B, double max_correspondence_distance, int max_iteration,
                       double relative_fitness, double relative_rmse, int estimation, const double* tgt_normals,
                       double* out_transform, double* out_stats, const pcrcg_icp_trace_ex* trace, void* ws, size_t ws_bytes,
                       void* stream);

/* Generalized ICP: batched plane-to-plane refinement (csrc/icp.hip, csrc/gicp_terms.h; added under ABI version 4, which it
 * does not change) -- Segal, Haehnel, Thrun, "Generalized-ICP" (RSS 2009); open3d's registration_generalized_icp with
 * TransformationEstimationForGeneralizedICP(epsilon), restated as a deterministic algorithm; no bit parity with open3d is
 * claimed.  This comment is the definition, DESIGN.md section 23 explains it, tests/gicp_ref.py restates it in numpy.
 *
 * pcrcg_covariances_from_normals: normals [n, 3] f64 DEVICE -> cov [n, 6] f64 DEVICE = (xx, xy, xz, yy, yz, zz), the packing
 *   of pcrcg_estimate_normals_batch's cov, of C = I - (1 - epsilon) n n^T: a disc of unit extent in the tangent plane and
 *   epsilon along the normal.  s = 1.0 - epsilon; a_r = s n_r; entry (r, c) = (r == c ? 1.0 : 0.0) - a_r n_c, in float64,
 *   every operation rounded separately.  For a unit normal this is open3d's Rot diag(epsilon, 1, 1) Rot^T, and its
 *   U diag(1, 1, epsilon) U^T from the neighbourhood covariance's SVD (sum u_i u_i^T = I).  It is even in n, bit for bit.  A
 *   normal that is not finite gives entries that are not finite (they propagate: see Update).  One thread per row.
 *   epsilon outside (0, 1] or NaN, a negative n, and a null normals / cov with n > 0 give PCRCG_EBADARG; n = 0 launches nothing.
 *
 * pcrcg_gicp_batch: layout, grid, init, n_max, the outputs, the statistics, the NaN rules, empty pairs, the `done` word and
 *   the launch count are pcrcg_icp_batch's.
 *   src_cov [n_total, 6] and tgt_cov [m_total, 6] f64 DEVICE, in the clouds' row order, packed as above; each is required
 *     unless its side has no rows.  The source's covariances belong to the UNMOVED source cloud: the kernel rotates them.
 *   Evaluate(T) is pcrcg_icp_batch's -- the same moved fp32 point, nearest target, lowest-index tie rule, count, fitness and
 *     Euclidean rmse -- and convergence is tested on those values, as open3d's loop does.
 *   Update: over the correspondences (i -> j), with p the moved source point (the float64 value of the fp32 result), q its
 *     target and R the rotation block of T_k in float64 (row-major r00 .. r22), every operation in float64 and rounded
 *     separately (csrc/gicp_terms.h):
 *       X = R C_s[i], the full 3 x 3: X[r][c] = ((R[r][0] S[0][c] + R[r][1] S[1][c]) + R[r][2] S[2][c]);
 *       M = C_t[j] + X R^T, six entries r <= c: M[r][c] = C_t[r][c] + ((X[r][0] R[c][0] + X[r][1] R[c][1]) + X[r][2] R[c][2]);
 *       W = M^-1 by the adjugate: c00 = m11 m22 - m12 m12, c01 = m02 m12 - m01 m22, c02 = m01 m12 - m02 m11,
 *         c11 = m00 m22 - m02 m02, c12 = m01 m02 - m00 m12, c22 = m00 m11 - m01 m01, det = ((m00 c00 + m01 c01) + m02 c02),
 *         W = c / det (six divisions);
 *       d = p - q; J0 = [-[p]x | I] (3 x 6), the rows of -[p]x being (0, pz, -py), (-pz, 0, px), (py, -px, 0): fast global
 *         registration's Jacobian, about the origin;
 *       with w_r the rows of W: g_r = p x w_r (the rows of W (-[p]x); a cross product is a b - c d per component); the
 *         rotation block of J0^T W J0, row a and columns c >= a: the a-th component of p x (g_0[c], g_1[c], g_2[c]); the mixed
 *         block [a][3 + c] = g_c[a]; the translation block = W; e_r = ((w_r0 d0 + w_r1 d1) + w_r2 d2); the terms of the right
 *         side are -(p x e) and -e.
 *     A = sum J0^T W J0 (the 21 entries of the upper triangle, row by row) and b = -sum J0^T W d (6), in float64 and in the
 *     fixed order of the other sums (shuffle tree, the eight wavefronts in order, the workgroups in order).  A x = b is solved
 *     by pcrcg_icp_batch_ex's LDL^T (csrc/smallsolve.h, its 1e-12 pivot rule) in the one lane that runs the other fits;
 *     delta = Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5) and T <- delta T, as point-to-plane's.
 *     The pair stops, keeping T, if count < 3 or the solve is refused.  A bad M has no special case: a covariance that is not
 *     finite, or det M = 0 (zero covariances on both sides), makes the pair's sums not finite, the solve refuses and the pair
 *     stops as a degenerate one -- the rule of a normal that is not finite in point-to-plane.  A row that is nobody's
 *     correspondence is not read.
 *   With C_s = C_t = I (epsilon = 1) the update is a Gauss-Newton step of point-to-point; nothing depends on the covariances'
 *     common scale but the size of W.
 *   Range: J0 takes the moved point about the ORIGIN, as point-to-plane's J does, so A's rotation block grows with |p|^2 and
 *     cond(A) with (distance from the origin / extent of the cloud)^2; the pivot rule refuses a pair that is far enough out,
 *     and callers re-centre such clouds ("Range" of pcrcg_icp_batch_ex; DESIGN.md section 23 has the numbers).
 *   trace: pcrcg_icp_trace_ex's members; sums27 [B, max_iteration + 1, 27] = A's upper triangle then b of Evaluate(T_k).
 *   Workspace: pcrcg_gicp_batch_ws_bytes(B, n_total, m_total, max_iteration) = pcrcg_icp_batch_ex_ws_bytes' value (28 terms a
 *   slot); 0 as pcrcg_icp_batch_ws_bytes.  Bad arguments (pcrcg_icp_batch's, a missing src_cov with n_total > 0 or tgt_cov with
 *   m_total > 0) give PCRCG_EBADARG, a short workspace PCRCG_EWORKSPACE, before anything launches. */
int pcrcg_covariances_from_normals(const double* normals, long n, double epsilon, double* cov, void* stream);
size_t pcrcg_gicp_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration);
int pcrcg_gicp_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                     const void* grid, const double* init, int B, double max_correspondence_distance, int max_iteration,
                     double relative_fitness, double relative_rmse, const double* src_cov, const double* tgt_cov,
                     double* out_transform, double* out_stats, const pcrcg_icp_trace_ex* trace, void* ws, size_t ws_bytes,
                     void* stream);

/* Colored ICP: batched joint colour / geometry refinement (csrc/colored.hip, csrc/icp.hip, csrc/colored_terms.h; added under
 * ABI version 4, which it does not change) -- Park, Zhou, Koltun, "Colored Point Cloud Registration Revisited" (ICCV 2017);
 * open3d 0.10's registration_colored_icp (ColoredICP.cpp), restated as a deterministic algorithm; no bit parity with open3d is
 * claimed.  This comment is the definition, DESIGN.md section 24 explains it, tests/colored_icp_ref.py restates it in numpy.
 * The intensity of a point is I = ((r + g) + b) / 3.0 in float64; the entries take intensities, not colours.
 *
 * pcrcg_color_gradients_batch: the colour gradients of B ragged (target) clouds in ONE launch, open3d's
 *   InitializePointCloudForColoredICP.  One wavefront per point.
 *   Layout: pts, off, n_max and grid as pcrcg_estimate_normals_batch (the grid is built at THIS radius); open3d passes
 *   radius = 2 max_correspondence_distance and max_nn = 30.  normals [n_total, 3] f64 and intensity [n_total] f64 DEVICE, in the
 *   clouds' row order, required.
 *   Outputs: rec [n_total, 8] f64, one packed 64-byte record per point: (n [3], g [3], I, 0) -- the point's normal and
 *   intensity as they were given, and its gradient g -- which pcrcg_colored_icp_batch reads with one aligned load per
 *   correspondence; optional (NULL: not written), for tests: count [n_total] i32 and sums [n_total, 9] f64.
 *   Definition, per point k of a cloud with vt = (double)p_k, nt its normal, in float64, every operation rounded separately,
 *   dot products as ((x + y) + z) (csrc/colored_terms.h):
 *     Neighbours: exactly the list of "Normal estimation" above (fp32 unfused d2 < (float)radius * (float)radius, ascending
 *       (d2, cloud-local index), cut to the first max_nn); nn = its length = count.
 *     nn < 4: g = 0 and sums = 0.
 *     Otherwise the entries e = 1 .. nn - 1 (entry 0 is dropped whichever point it is: for distinct points it is k itself, among
 *       coincident points it is the lowest index), with a = (double)p_e: dot = ((a - vt) . nt); A_e = (a - dot nt) - vt,
 *       b_e = I[a] - I[k]; the row adds (A0 A0, A0 A1, A0 A2, A1 A1, A1 A2, A2 A2, A0 b, A1 b, A2 b).  Lane e of the wavefront
 *       holds entry e's nine products (zero elsewhere) and a 64-lane shuffle tree adds them: a function of the row alone.  No
 *       floating-point atomics.
 *     Last row (nn - 1) nt with right side 0: w = (double)(nn - 1), r = w nt, and r_r r_c is added to the six entries of A^T A.
 *       sums = A^T A's upper triangle (00 01 02 11 12 22), then A^T b, at this point.
 *     g = the solution of (A^T A) g = A^T b by LDL^T with diagonal pivoting (csrc/smallsolve.h solve_ldlt3: pcrcg_icp_batch_ex's
 *       solve with 6 read as 3, the same 1e-12 pivot rule); a refused solve gives g = 0.
 *   NaN rules: an intensity that is not finite makes b, and so g, not finite in every row whose entries 1 .. nn - 1 hold the
 *     point, and in the point's own row; every other row keeps its bits.  A normal that is not finite makes A^T A not finite,
 *     the solve refuses, and the row gets g = 0 beside the normal as given.
 *   A row's bits depend on its cloud's points, normals and intensities alone.  The entry allocates nothing, synchronises
 *   nothing and reads nothing back.  The argument rules are pcrcg_estimate_normals_batch's (max_nn in 1..64), with normals,
 *   intensity and rec required when n_total > 0.  Workspace: pcrcg_color_gradients_ws_bytes(B, n_total) (256 bytes today: the
 *   lists live in LDS); 0 for B outside 1..65535 or a negative n_total.
 *
 * pcrcg_colored_icp_batch: layout, grid, init, n_max, the outputs, the statistics, empty pairs, the `done` word and the launch
 *   count are pcrcg_icp_batch's.
 *   lambda_geometric in [0, 1] (open3d: 0.968): sg = sqrt(lambda_geometric), sp = sqrt(1.0 - lambda_geometric), on the host.
 *   tgt_rec [m_total, 8] f64 DEVICE: the targets' records above, 64-byte aligned; src_intensity [n_total] f64 DEVICE; each is
 *     required unless its side has no rows.
 *   Evaluate(T) is pcrcg_icp_batch's -- the same moved fp32 point, nearest target, lowest-index tie rule, count, fitness and
 *     Euclidean (point-to-point) rmse -- and convergence is tested on those values, as open3d's loop does.
 *   Update: over the correspondences (i -> j), with p the moved source point (the float64 value of the fp32 result), q its
 *     target, (n, g, It) the target's record and Is = src_intensity[i] (csrc/colored_terms.h):
 *       rG = ((p - q) . n); J = [p x n | n] (a cross product is a b - c d per component); JG = sg J, rg = sg rG;
 *       e = (p - rG n) - q; I0 = ((g . e)) + It; ri = sp (Is - I0);
 *       gn = ((g . n)); gM = -(g - gn n); JI = sp [p x gM | gM];
 *       the 27 terms: JG_r JG_c + JI_r JI_c over the upper triangle row by row (21), then -(JG_r rg + JI_r ri) (6).
 *     They are added in float64 in the fixed order of the other sums (shuffle tree, the eight wavefronts in order, the
 *     workgroups in order); A x = b is solved by pcrcg_icp_batch_ex's LDL^T (its 1e-12 pivot rule) in the one lane that runs the
 *     other fits; delta = Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5) and T <- delta T, as point-to-plane's.
 *     The pair stops, keeping T, if count < 3 (every correspondence carries two equations), if an entry of b is not finite
 *     (an intensity touches b alone, which the pivots never see) or if the solve is refused: anything degenerate is for the
 *     pivot rule to refuse.
 *   With lambda_geometric = 1 and finite records and intensities, the terms are point-to-plane's as values (sp = 0), and a pair
 *     whose count stays >= 6 gets pcrcg_icp_batch_ex(estimation = 1)'s outputs.
 *   NaN rules: a record or an intensity that is not finite in a row that IS a correspondence makes the pair's sums not finite,
 *     the solve refuses (or b fails its test) and the pair stops with T kept; a row that is nobody's correspondence is not read and changes nothing.
 *     The other NaN rules are pcrcg_icp_batch's.
 *   Range: J takes the moved point about the ORIGIN, as point-to-plane's does, so A's rotation block grows with |p|^2 and
 *     cond(A) with (distance from the origin / extent of the cloud)^2; the pivot rule refuses a pair that is far enough out,
 *     and callers re-centre such clouds ("Range" of pcrcg_icp_batch_ex).
 *   trace: pcrcg_icp_trace_ex's members; sums27 [B, max_iteration + 1, 27] = A's upper triangle then b of Evaluate(T_k).
 *   Workspace: pcrcg_colored_icp_batch_ws_bytes(B, n_total, m_total, max_iteration) = pcrcg_icp_batch_ex_ws_bytes' value; 0 as
 *   pcrcg_icp_batch_ws_bytes.  Bad arguments (pcrcg_icp_batch's, lambda_geometric outside [0, 1] or NaN, a missing
 *   src_intensity with n_total > 0 or tgt_rec with m_total > 0) give PCRCG_EBADARG under this entry's name, a short workspace
 *   PCRCG_EWORKSPACE, before anything launches. */
size_t pcrcg_color_gradients_ws_bytes(int B, int n_total);
int pcrcg_color_gradients_batch(const float* pts, const int* off, int n_total, int n_max, const void* grid, int B, double radius,
                                int max_nn, const double* normals, const double* intensity, double* rec, int* count, double* sums,
                                void* ws, size_t ws_bytes, void* stream);
size_t pcrcg_colored_icp_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration);
int pcrcg_colored_icp_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                            const void* grid, const double* init, int B, double max_correspondence_distance, int max_iteration,
                            double relative_fitness, double relative_rmse, double lambda_geometric, const double* tgt_rec,
                            const double* src_intensity, double* out_transform, double* out_stats,
                            const pcrcg_icp_trace_ex* trace, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Robust kernels
 * Point-to-plane and colored ICP under a robust loss kernel (csrc/icp.hip, csrc/robust_kernel.h, csrc/colored_terms.h; added
 * under ABI version 4, which it does not change) -- open3d's RobustKernel passed to TransformationEstimationPointToPlane and
 * TransformationEstimationForColoredICP: every row of the Gauss-Newton system is multiplied with a weight of its own
 * residual, so that the correspondences inside the gate which are not true matches (another surface, a moving object) pull
 * the step less than the true ones do.  This comment is the definition, tests/robust_ref.py restates it in numpy.
 *
 *   kernel (the kind) and kernel_k (its scale k, in the residual's unit) are shared by all pairs of a call.  The weight of a
 *   residual r, in float64, basic IEEE operations in the order written (csrc/robust_kernel.h robust_weight):
 *     0 L2      1.0
 *     1 L1      1.0 / max(|r|, 1e-12)
 *     2 Huber   k / max(|r|, k)
 *     3 Cauchy  1.0 / (1.0 + (r / k) (r / k))
 *     4 GM      k / ((k + r r) (k + r r))
 *     5 Tukey   t = min(1.0, |r| / k); u = 1.0 - t t; u u
 *   max and min keep a NaN: a residual that is not a number gives a weight that is not a number (L2: 1.0), an infinite one 0.
 *   The L1 floor (kL1Floor = 1e-12) is the one departure from open3d, whose L1 weight is 1 / |r|: infinite for a
 *   correspondence that lies exactly on its target's plane, where it turns the pair's system into NaN.
 *
 * pcrcg_icp_plane_robust_batch: pcrcg_icp_batch_ex(estimation = 1) -- every argument, rule and output -- with the terms of a
 *   correspondence, res = ((p - q) . n) and J = [p x n | n] as there, w = weight(res):
 *     w (J_r J_c) over the upper triangle row by row (21), then w (-(J_r res)) (6).
 *   The weight multiplies the finished term of the plain estimator: kernel 0 gives pcrcg_icp_batch_ex's bits.
 * pcrcg_colored_icp_robust_batch: pcrcg_colored_icp_batch -- every argument, rule and output -- with the two rows of a
 *   correspondence weighted separately on their scaled residuals, as open3d does, wg = weight(rg), wi = weight(ri):
 *     wg (JG_r JG_c) + wi (JI_r JI_c) over the upper triangle (21), then -(wg (JG_r rg) + wi (JI_r ri)) (6).
 *   Kernel 0 gives pcrcg_colored_icp_batch's bits.
 * What stays unweighted, in both: the correspondence search and the gate, the count, the d2 sum, fitness and the Euclidean
 *   rmse and so the convergence test; the count < 6 (colored: count < 3) rule; colored ICP's finiteness test of b; the
 *   order of the sums; the LDL^T solve with its 1e-12 pivot rule; the delta.  A system that the weights make singular --
 *   Tukey with every |r| >= k: all weights 0 -- or not finite is refused by the solve and the pair stops with T kept, as any
 *   degenerate pair does.
 *   trace: pcrcg_icp_trace_ex's members; sums27 holds the WEIGHTED sums.
 *   Workspace: the *_ws_bytes of the plain entries' values.  Bad arguments: the plain entry's, a kernel outside 0..5, and for
 *   kernels 2..5 a kernel_k that is not positive and finite (NaN included; kernels 0 and 1 do not read kernel_k), give
 *   PCRCG_EBADARG under the robust entry's name; a short workspace PCRCG_EWORKSPACE, before anything launches.
 *   Generalized ICP has no robust entry: open3d weights the three rows of M^(-1/2) d separately, which takes the inverse
 *   square root of the 3 x 3 metric per correspondence -- another term computation than csrc/gicp_terms.h's J0^T W J0. */
size_t pcrcg_icp_plane_robust_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration);
int pcrcg_icp_plane_robust_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                                 const void* grid, const double* init, int B, double max_correspondence_distance,
                                 int max_iteration, double relative_fitness, double relative_rmse, const double* tgt_normals,
                                 int kernel, double kernel_k, double* out_transform, double* out_stats,
                                 const pcrcg_icp_trace_ex* trace, void* ws, size_t ws_bytes, void* stream);
size_t pcrcg_colored_icp_robust_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration);
int pcrcg_colored_icp_robust_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                                   const void* grid, const double* init, int B, double max_correspondence_distance,
                                   int max_iteration, double relative_fitness, double relative_rmse, double lambda_geometric,
                                   const double* tgt_rec, const double* src_intensity, int kernel, double kernel_k,
                                   double* out_transform, double* out_stats, const pcrcg_icp_trace_ex* trace, void* ws,
                                   size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fast global registration
 * The other half of the classical global-registration recipe that FPFH feeds: Zhou, Park, Koltun, "Fast Global
 * Registration" (ECCV 2016), open3d's registration_fast_based_on_feature_matching, for B ragged pairs in one launch
 * (csrc/fgr.hip; added under ABI version 4, which it does not change).  open3d draws its tuples with rand(), so this is a
 * deterministic algorithm of the same structure; no bit parity with open3d is claimed.  This comment is the definition,
 * DESIGN.md section 22 explains it and tests/fgr_ref.py restates it in numpy float64.
 *
 * pcrcg_mutual_match_batch: the mutual L2 correspondences of B pairs.  Layout, argument checks and conventions are
 * pcrcg_feature_match_batch's.
 *   nn_s(i) = pcrcg_feature_match_batch's row i: the arg-max over j of <a_i, b_j> - |b_j|^2 / 2 in fp32, lowest index on ties;
 *   nn_t(j) = the same rule with the roles exchanged: the arg-max over i of <b_j, a_i> - |a_i|^2 / 2, lowest index on ties.
 *   Pair b's list holds the (i, nn_s(i)) with nn_t(nn_s(i)) == i in ascending i, written from row src_off[b] of
 *   corr [n_total, 2] i32 with indices local to the pair; k[b] is its length; rows k[b] .. n_b - 1 of the pair are written as
 *   (-1, -1).  A pair with n_b = 0 or m_b = 0 gets k[b] = 0.  (FPFH rows are not normalised, so the inner-product arg-max of
 *   pcrcg_feature_match's mutual = 1 is not their L2 neighbour; this is.)
 *   Workspace: pcrcg_mutual_match_batch_ws_bytes(B, n_total, m_total) = 12 (n_total + m_total) bytes plus alignment padding;
 *   0 for B outside 1..65535 or a negative size.  Nothing is allocated, synchronised or read back.
 *
 * pcrcg_fgr_batch: src [n_total, 3] / tgt [m_total, 3] f32 and src_off / tgt_off [B + 1] i32 DEVICE row offsets as
 * pcrcg_ransac_batch's; corr [n_total, 2] i32 and k [B] i32 as pcrcg_mutual_match_batch or pcrcg_feature_match_batch write
 * them, or the caller's own (pair b's rows start at src_off[b], indices local to the pair; like pcrcg_ransac_batch the entry
 * trusts them).  seeds [B] u64 DEVICE, each < 2^24.  Every parameter is shared by the pairs of a call.
 * Per pair b, independent of every other pair, with P = min(max(k[b], 0), n_b) (0 when a side of the pair is empty) and
 * delta = maximum_correspondence_distance:
 *   Tuple stage.  tuple_scale == 0: skipped; E = the first min(P, 3 maximum_tuple_count) rows of the list, in order (the
 *     statistics report 0 tuples and 0 trials).  Otherwise trial t = 0 .. 100 P - 1 (64-bit) draws the three rows
 *     ((r >> 32) * P) >> 32, r = splitmix64((seed << 40) + 4 t + s), s < 3 (splitmix64 as in "Registration back end").  With
 *     p_0..p_2 the drawn source points and q_0..q_2 the drawn target points widened to float64, and for the edges (0,1), (1,2),
 *     (2,0): li = sqrt((dx dx + dy dy) + dz dz) over the p, lj likewise over the q.  The trial passes iff
 *     li * tuple_scale < lj and lj * tuple_scale < li for all three edges (a repeated row gives li = 0 and fails by itself).
 *     The first maximum_tuple_count passing trials in ascending t are accepted; E = their rows, three per trial, in trial
 *     order, duplicates kept.  trials_used = (last accepted t) + 1 when the cap is reached, else 100 P.
 *   Frame.  |E| < 10: the identity, updates = 0, mu = 0, share = 0.  Otherwise cs = (sum_e p_e) / |E|, ct = (sum_e q_e) / |E|
 *     in float64; p~ = p - cs, q~ = q - ct; D2 = max_e max(|p~_e|^2, |q~_e|^2), |v|^2 = (x x + y y) + z z; mu = D2.  D2 zero or
 *     not finite: the identity, updates = 0, mu = D2, share = 0.
 *   Iterations it = 0 .. iteration_number - 1, T = [R|t] float64 from the identity.  Moved point
 *     p = ((R0 x + R1 y) + R2 z) + t0 of p~ (and likewise the other components), r = p - q~, weight
 *     l = (mu / (|r|^2 + mu))^2.  J_x = (0, p_z, -p_y, 1, 0, 0), J_y = (-p_z, 0, p_x, 0, 1, 0), J_z = (p_y, -p_x, 0, 0, 0, 1);
 *     A = sum l (J_x J_x^T + J_y J_y^T + J_z J_z^T) (the 21 entries of the upper triangle, row by row) and
 *     g = -sum l (J_x r_x + J_y r_y + J_z r_z) (6), in float64 and in a fixed order: per thread over its entries
 *     e = thread, thread + 512, ..., a shuffle tree inside each wavefront, the eight wavefronts in order.  No floating-point
 *     atomics.  x = the LDL^T solve of A x = g (csrc/smallsolve.h, pcrcg_icp_batch_ex's): on failure the loop ends and T is
 *     kept; otherwise delta = Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5) as pcrcg_icp_batch_ex's update, T <- delta T, updates += 1,
 *     and then, if decrease_mu and it % 4 == 0 and mu > delta^2, mu <- mu / division_factor.
 *   Output.  R_out = R, t_out = (t - R cs) + ct with R cs as ((r0 x + r1 y) + r2 z).  out_transform [B, 16] f64 row-major;
 *     out_stats [B, 6] f64 = (P, tuples accepted, trials_used, updates, final mu, the share of E's entries with |r|^2 < delta^2
 *     at the final T).  A pair whose seed is >= 2^24 gets NaN in all 22 outputs, as in pcrcg_ransac_batch.
 *   Departures from open3d 0.10: the source is moved, so the result maps source onto target and no final inverse is taken;
 *     everything is in the clouds' own units and mu runs from D2 towards delta^2 as in the paper (open3d's normalised-unit
 *     distance and its distance-versus-squared-distance comparison are not reproduced); centroids and D are taken over E, not
 *     over the clouds; the edge test multiplies by the scale on both sides, as RANSAC's edge-length checker; rand() is
 *     replaced by the counter-based draws above.
 *   trace (NULL, or any member NULL: not written), for tests: trials [B, maximum_tuple_count] i64 the accepted trial ids,
 *     entries [B, 3 maximum_tuple_count, 2] i32 = E, frame [B, 7] f64 = cs, ct, D2 (written when |E| >= 10), and per iteration
 *     that ran transforms [B, iteration_number, 16] f64 = T before the step, mu [B, iteration_number] f64 = mu before the
 *     step, sums27 [B, iteration_number, 27] f64 = A's upper triangle then g.  What is not reached keeps what it held.
 *   One launch, one workgroup of 512 threads per pair: every loop is bounded by what the host passes (100 P <= 100 n_b
 *   trials, iteration_number steps) and no workgroup waits for another.  Workspace:
 *   pcrcg_fgr_batch_ws_bytes(B, n_total, maximum_tuple_count, iteration_number) = 96 B maximum_tuple_count bytes plus
 *   alignment padding (today a function of B and maximum_tuple_count alone); 0 for arguments out of range.  Rejected with
 *   PCRCG_EBADARG before anything launches: null pointers (trace may be NULL), B outside 1..65535, delta <= 0 or not finite,
 *   division_factor <= 1, decrease_mu other than 0 or 1, iteration_number outside 1..65536, tuple_scale outside [0, 1],
 *   maximum_tuple_count outside 1..4096; a short workspace gives PCRCG_EWORKSPACE.  The entry allocates nothing and
 *   synchronises nothing.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pcrcg_fgr_trace {
    int64_t* trials;
    int* entries;
    double* frame;
    double* transforms;
    double* mu;
    double* sums27;
} pcrcg_fgr_trace;

size_t pcrcg_mutual_match_batch_ws_bytes(int B, int n_total, int m_total);
int pcrcg_mutual_match_batch(const float* src_feat, int ld_src, const int* src_off, int n_total, int n_max,
                             const float* tgt_feat, int ld_tgt, const int* tgt_off, int m_total, int m_max, int c, int B,
                             int* corr, int* k, void* ws, size_t ws_bytes, void* stream);
size_t pcrcg_fgr_batch_ws_bytes(int B, int n_total, int maximum_tuple_count, int iteration_number);
int pcrcg_fgr_batch(const float* src, const int* src_off, const float* tgt, const int* tgt_off, const int* corr, const int* k, int B,
                    double maximum_correspondence_distance, double division_factor, int decrease_mu, int iteration_number,
                    double tuple_scale, int maximum_tuple_count, const uint64_t* seeds, double* out_transform, double* out_stats,
                    const pcrcg_fgr_trace* trace, void* ws, size_t ws_bytes, void* stream);

/* Voxel down-sampling: open3d's PointCloud::VoxelDownSample for B ragged clouds in one set of launches (csrc/voxel.hip;
 * added under ABI version 4, which it does not change) -- what ref:datasets/kitti.py:134-140 does to both raw scans of a
 * pair before anything else sees them, and how raw 3DMatch fragments become the 2.5 cm clouds of ref:datasets/indoor.py.
 * It is NOT pcrcg_grid_subsample_batch: that grid starts at floor(min / dl) * dl and works in fp32; this one starts at
 * min - voxel_size / 2 and works in float64.  DESIGN.md section 14 defines it, tests/voxel_ref.py restates it in numpy.
 *   Layout: pts [n_total, 3] f32, the B clouds concatenated; off [B + 1] i32 DEVICE row offsets, never read by the host.
 *   out_pts [n_total, 3] f64 (capacity: the input rows); cloud b's rows follow cloud b-1's with no gap.  out_len [B] i32.
 *   out_first, out_count [n_total] i32, each optional (NULL: not written): per output row, the cloud-local index of the first
 *   input point of its voxel, and how many points the row averaged.
 *   Definition, per cloud; every step in IEEE float64 from the exactly widened fp32 coordinates, unfused:
 *     vmin = (min over the cloud) - 0.5 * voxel_size, per axis;  idx = (int)floor((p - vmin) / voxel_size), per axis;
 *     points with equal idx form a voxel; its row is (the sum of its points, added one by one in ascending input index,
 *     starting from 0.0) / (double)count.
 *   Row order: open3d emits rows in the iteration order of its hash map, an artefact of its hash and of the standard
 *     library it was built with.  That order is NOT reproduced, and -- as for pcrcg_icp_batch -- no bit parity with open3d
 *     is claimed.  Rows come in ascending index of each voxel's first input point.  The reference's consumers
 *     (get_correspondences, the collate function) take the down-sampled clouds as they come, so any fixed order is
 *     consistent downstream.
 *   Determinism: a cloud's output bits depend on its own points and voxel_size alone -- not on B, its position in the batch
 *     or the run.  There are no floating-point atomics: one thread adds a voxel's points in order (a cloud that falls into
 *     one voxel is slow but correct).
 *   Rejected clouds get out_len[b] = -1 and no rows, and affect no other cloud: a cloud with a non-finite coordinate, and a
 *     cloud whose index on any axis would reach 2^21, the limit of the key packing (open3d's "voxel_size is too small").
 *   An empty cloud gets out_len[b] = 0.  Offsets that do not describe a range inside n_total (off[b] < 0, off[b] >
 *     off[b + 1], off[b + 1] > n_total), or that step back over an earlier accepted range, read as an empty cloud.
 *   Rows of out_pts / out_first / out_count past the last one written keep what they held.
 *   The entry allocates nothing, synchronises nothing and enqueues everything (at most 12 launches) at once on `stream`.
 *   Null pts / off / out_pts / out_len / ws, B outside 1..65535, n_total < 0 or above 2^30, and a voxel_size that is not
 *   finite or not positive are rejected with PCRCG_EBADARG before any launch; a short workspace with PCRCG_EWORKSPACE.
 *   Workspace: pcrcg_voxel_down_sample_ws_bytes(B, n_total), about 68 bytes per row; 0 for the same bad sizes. */
size_t pcrcg_voxel_down_sample_ws_bytes(int B, int n_total);
int pcrcg_voxel_down_sample_batch(const float* pts, const int* off, int n_total, int B, double voxel_size, double* out_pts,
                                  int* out_len, int* out_first, int* out_count, void* ws, size_t ws_bytes, void* stream);

/* Interest-point sampler: weighted sampling without replacement of S ragged segments in ONE launch, the step between the
 * network's overlap x saliency scores and pcrcg_feature_match_batch (the reference draws it on the host with
 * np.random.choice(..., replace=False, p = scores / sum), ref:lib/tester.py:152-164).  The distribution is that draw's
 * (successive sampling proportional to the scores); the stream is this library's own, specified here, in DESIGN.md
 * section 10 and in tests/sample_ref.py.
 *   Layout: scores [n_total] f32, the segments concatenated; seg_off [S + 1] i32 DEVICE row offsets (seg_off[0] = 0,
 *   non-decreasing); seeds [S] u64 DEVICE, each < 2^24; out_off [S + 1] i32 DEVICE = the prefix sums of
 *   min(N_s, n_keep), which the caller computes (it knows the lengths); out_idx [out_off[S]] i32.
 *   For segment s with N rows, scores w_i and seed sd:
 *     h_i   = splitmix64(splitmix64((sd << 40) + i) ^ 0x53414D504C455231)      (splitmix64 as above; the constant keeps
 *             the stream apart from the one pcrcg_ransac draws from under the same seed)
 *     u_i   = ((double)(h_i >> 11) + 0.5) * 2^-53                               (IEEE double, round to nearest even)
 *     key_i = -log(u_i) / (double)w_i  for a finite w_i > 0, +inf otherwise
 *   N <= n_keep: every row is kept.  Otherwise the n_keep rows with the smallest keys are kept, equal keys (also the +inf
 *   keys of a segment with fewer than n_keep positive scores) in ascending row order.  out_idx[out_off[s] ..] receives the
 *   kept rows, local to the segment, in ascending order.  A segment's result depends on its own scores, n_keep and seed
 *   only -- not on S, on its position, or on the schedule (no floating-point atomics) -- and is the same bits every run.
 *   The offsets and seeds are not read by the host: an empty segment, or one whose offsets do not lie within the rows the
 *   workspace was sized for, writes nothing, and a segment whose seed is >= 2^24 gets -1 in all of its outputs.
 * Workspace: pcrcg_weighted_sample_ws_bytes(S, n_total) = 8 n_total bytes plus alignment padding (the keys); 0 for S < 1 or
 * a negative total.  One workgroup per segment, rows walked in strides of it: any segment length.  The entry allocates
 * nothing and synchronises nothing; null pointers, S < 1 and n_keep < 1 are rejected with PCRCG_EBADARG before anything
 * launches. */
size_t pcrcg_weighted_sample_ws_bytes(int S, int n_total);
int pcrcg_weighted_sample_batch(const float* scores, const int* seg_off, int S, int n_keep, const uint64_t* seeds, int* out_idx,
                                const int* out_off, void* ws, size_t ws_bytes, void* stream);

/* Inlier statistics of many pairs: the inlier ratio and its mutual variant (ref:lib/benchmark_utils.py:226-267,
 * get_inlier_ratio) of B ragged pairs in one set of launches, the inputs of feature-match recall.
 *   Layout: as pcrcg_feature_match_batch's -- src [n_total, 3], tgt [m_total, 3] f32, descriptors [n_total, c] /
 *   [m_total, c] with row strides ld_src / ld_tgt, src_off / tgt_off [B + 1] i32 DEVICE row offsets, n_max / m_max (host)
 *   >= every pair's source / target length.  rt [B, 12] f32 DEVICE: pair b's ground-truth R (row-major) then t.
 *   thr [n_thr] f32 HOST: the distance thresholds, 1 <= n_thr <= 32.
 *   For pair b, both arg-max directions of <a_i, b_j>: arg_s[i] = argmax_j, arg_t[j] = argmax_i, lowest index on ties --
 *   each row bit for bit what pcrcg_feature_argmax gives on that pair alone (the same device code and kernel choice).
 *   Then for every source row i: p = R src_i + t in unfused fp32, ((r0 x + r1 y) + r2 z) + t0 (RANSAC's evaluation
 *   arithmetic), d_i = sqrtf((dx dx + dy dy) + dz dz) with dx = p - tgt[arg_s[i]] and a correctly rounded square root,
 *   mutual_i = (arg_t[arg_s[i]] == i) (the reference's mutual_selection);
 *     counts [B, 2, n_thr] i32: [b, 0, k] = #{i : d_i < thr[k]} ("wo"), [b, 1, k] = #{i : mutual_i and d_i < thr[k]} ("w");
 *     k_mutual [B] i32 = #{i : mutual_i}.
 *   The comparison is in fp32 against the fp32 threshold.  All counts are integers, so the result does not depend on
 *   the order of the pairs, on B or on the schedule.  Optional outputs (NULL: not written), pair b's rows at src_off[b] /
 *   tgt_off[b], indices local to the pair: dist [n_total] f32 = d_i (NaN for a pair without targets), mutual [n_total]
 *   i32 0/1, arg_s [n_total] i32, arg_t [m_total] i32.
 * Workspace: pcrcg_inlier_stats_batch_ws_bytes(B, n_total, m_total) = 8 (n_total + m_total) bytes plus alignment padding;
 * 0 for B outside 1..65535 or an empty total.  The entry zeroes counts and k_mutual itself, allocates nothing and
 * synchronises nothing.  Bad arguments (null pointers, B outside 1..65535, n_thr outside 1..32, a NaN threshold, sizes
 * that contradict each other) are rejected with PCRCG_EBADARG and a short workspace with PCRCG_EWORKSPACE, before
 * anything launches; the offsets live on the device and are not read by the host. */
size_t pcrcg_inlier_stats_batch_ws_bytes(int B, int n_total, int m_total);
int pcrcg_inlier_stats_batch(const float* src, const float* src_feat, int ld_src, const int* src_off, int n_total, int n_max,
                             const float* tgt, const float* tgt_feat, int ld_tgt, const int* tgt_off, int m_total, int m_max,
                             int c, int B, const float* rt, const float* thr, int n_thr, int* counts, int* k_mutual,
                             float* dist, int* mutual, int* arg_s, int* arg_t, void* ws, size_t ws_bytes, void* stream);


/* Modified Chamfer distance of many pairs: the heavy part of the ModelNet evaluation's compute_metrics
 * (ref:lib/tester.py:280-286) for B ragged pairs in one set of launches, nothing materialised.
 *   Layout: as pcrcg_inlier_stats_batch's -- src [n_total, 3] (points_src), ref [m_total, 3] (points_ref), raw
 *   [r_total, 3] (points_raw, the clean cloud) f32; src_off / ref_off / raw_off [B + 1] i32 DEVICE row offsets; pred, gt
 *   [B, 12] f32 DEVICE: pair b's predicted and ground-truth R (row-major) then t.  For pair b:
 *     d_src[i] = min_j |pred src_i - raw_j|^2                 arg_src[i] = the j that attains it
 *     d_ref[i] = min_j |ref_i - (pred o gt^-1) raw_j|^2       arg_ref[i] = the j that attains it
 *     mean_src[b] = mean(d_src), mean_ref[b] = mean(d_ref), chamfer[b] = mean(d_src) + mean(d_ref).
 *   Arithmetic: a point is moved in unfused fp32, ((r0 x + r1 y) + r2 z) + t0 (RANSAC's evaluation arithmetic; the source
 *   points once each, the clean cloud once per query tile while it is staged).  pred o gt^-1 is composed ONCE per pair
 *   the way the reference composes it -- R = Rp Rg^T, t = Rp (-(Rg^T tg)) + tp -- in float64 from the fp32 poses and
 *   rounded to fp32 once.  The squared distance is (dx dx + dy dy) + dz dz in unfused fp32; the minimum over j is exact;
 *   arg_* is the LOWEST j that attains it, local to the pair.  The means: the fp32 minima are added in float64 in a fixed
 *   order (256 rows per workgroup by a fixed tree, the workgroups' partials in row order by a second kernel; no
 *   floating-point atomics), divided by the row count in float64 and rounded to fp32; chamfer is the float64 sum of the two
 *   float64 means rounded to fp32.  So pair b's three results and its per-point outputs are bit-identical whether the
 *   pair is evaluated alone, at any position of a batch, or twice.
 *   A row whose distances include a NaN (a NaN coordinate on either side after the transform, or infinities of one sign
 *   in one coordinate on both) gets d = NaN (torch.min's rule) and arg = -1, and so do the rows of a pair whose
 *   points_raw is empty.  A pair in which any of the three clouds is empty gets NaN in chamfer, mean_src and mean_ref.
 *   NaNs stay inside their pair.  Optional (NULL: not written): mean_src, mean_ref [B]; d_src, arg_src [n_total]; d_ref,
 *   arg_ref [m_total] (pair b's rows at src_off[b] / ref_off[b]).
 * Workspace: pcrcg_chamfer_batch_ws_bytes(B, n_total, m_total, r_total) = 8 ((n_total >> 8) + (m_total >> 8) + 2 B + 2)
 * bytes plus alignment padding (one float64 partial per workgroup); 0 for B outside 1..65535 or a negative total.  The
 * entry allocates nothing and synchronises nothing.  Bad arguments (null pointers, B outside 1..65535, negative totals)
 * are rejected with PCRCG_EBADARG and a short workspace with PCRCG_EWORKSPACE, before anything launches; the offsets live
 * on the device and are not read by the host (the launch is sized from the totals; a pair whose offsets do not describe
 * a range inside its stack reads as empty). */
size_t pcrcg_chamfer_batch_ws_bytes(int B, int n_total, int m_total, int r_total);
int pcrcg_chamfer_batch(const float* src, const int* src_off, int n_total, const float* ref, const int* ref_off, int m_total,
                        const float* raw, const int* raw_off, int r_total, int B, const float* pred, const float* gt,
                        float* chamfer, float* mean_src, float* mean_ref, float* d_src, int* arg_src, float* d_ref, int* arg_ref,
                        void* ws, size_t ws_bytes, void* stream);

/* PCR-CG's 2-D backbone Res50UNet(out_ch) (ref:models/resunet.py:163-188; the ResNet-50 encoder of ref:models/resnet.py and
 * the four up-projections of the decoder), forward only (the reference detaches it), enqueued by ONE call for n images.
 *   h_tensors / h_state: HOST array of n_tensors = 392 DEVICE pointers, the reference's state_dict order (every conv weight
 *   fp32 [cout][cin][kh][kw]; per BatchNorm2d weight, bias, running_mean, running_var f32 [C] and num_batches_tracked i64;
 *   decoder.conv0.bias last).
 *   pcrcg_res50unet_pack: the derived weight arena (pcrcg_res50unet_arena_bytes(out_ch) bytes): every convolution
 *   K-contiguous [cout][kh][kw][cin], the two 5x5 convolutions of each up-projection side by side as ONE [2 cout][25 cin]
 *   operand, the 7x7 stem as [64][160] (taps (ky, kx, ci), zero-padded).  Repack whenever a weight changes.
 *   pcrcg_res50unet_forward: images [n, 3, h, w] f32 (CHW) -> out [n, out_ch, 2 ceil(ceil(h/2)/2), 2 ceil(ceil(w/2)/2)]
 *   f32 (CHW; 120 x 160 at 240 x 320).  Every convolution runs as an implicit GEMM on the matrix cores with the forward
 *   products' arithmetic (pcrcg_gemm_set_mode, mode 1: the fp16 two-term split, and the three-term bf16 form for any tile
 *   that leaves fp16's normal range at either end); BatchNorm statistics come from fp64 column sums of the products.
 *     training = 1: batch statistics (biased variance, eps 1e-5) for the normalisation; running_mean / running_var are
 *       updated in place with momentum 0.1 and the unbiased variance.  joint_stats = 0: every image is its own batch of
 *       one (n updates, in image order; num_batches_tracked += n) -- PCR-CG's per-image calls; joint_stats = 1: one set of
 *       statistics over all n images (torch's training-mode BatchNorm2d on the batch; num_batches_tracked += 1).
 *     training = 0: the running statistics; nothing is written but out.
 *   Non-finite pixels or weights: the rule under "Point-wise blocks" -- the ReLU and the stem's max-pool keep NaN, so a
 *   poisoned input gives a non-finite output as in torch, never a finite one.
 *   Workspace: pcrcg_res50unet_ws_bytes(n, h, w) (0 for an unsupported shape).  Nothing is allocated or synchronised.
 *   Bad arguments (null pointers, n_tensors != 392, n outside 1..65535, h or w outside 1..8192, a training call in which a
 *   statistics segment would hold a single value) are rejected with PCRCG_EBADARG before anything launches. */
size_t pcrcg_res50unet_arena_bytes(int out_ch);
int pcrcg_res50unet_pack(void* const* h_tensors, int n_tensors, int out_ch, float* arena, void* stream);
size_t pcrcg_res50unet_ws_bytes(int n_images, int h, int w);
int pcrcg_res50unet_forward(const float* arena, void* const* h_state, int n_tensors, int out_ch, const float* images,
                            int n_images, int h, int w, int joint_stats, int training, float* out, void* ws, size_t ws_bytes,
                            void* stream);

/* Decoded RGB-D frames to the loader's tensors (ref:datasets/indoor.py:63-78: transforms.Resize(size, Image.NEAREST) +
 * transforms.ToTensor, and the depth frames' `/ 1000.0`), F colour and G depth frames in ONE launch (csrc/frames.hip).
 *   color [F, H, W, 3] uint8 (a decoded PNG's rows)  -> color_out [F, 3, oh, ow] f32 = (float)v / 255.0f;
 *   depth [G, Hd, Wd] uint16 (a 16-bit PNG's rows)   -> depth_out [G, ohd, owd] f32 = (float)(int16_t)v / 1000.0f.
 *   The int16 reading is the reference's: ToTensor takes PIL mode I;16 through np.int16, so the sensor's "no reading" value
 *   65535 becomes -0.001 and every raw value of 32768 or more comes out negative.  Both divisions are IEEE fp32 divisions.
 *   Nearest rule (PIL's Image.NEAREST, not torch's interpolate): output index i of an axis n_in -> n_out reads input index
 *   min(floor((i + 0.5) * n_in / n_out), n_in - 1), evaluated in float64.
 *   The colour frames of a call share one input and one output size, and so do the depth frames; either count may be 0 (its
 *   pointers and sizes are then ignored).  Plain stores, no atomics, no workspace; nothing is allocated or synchronised.
 *   Bad arguments (F + G outside 1..65535, a null pointer or a side outside 1..32768 of a kind whose count is not 0) are
 *   rejected with PCRCG_EBADARG before anything launches. */
int pcrcg_prepare_frames(const uint8_t* color, int F, int H, int W, int oh, int ow, float* color_out, const uint16_t* depth,
                         int G, int Hd, int Wd, int ohd, int owd, float* depth_out, void* stream);

/* ModelNet pair preparation: the data-parallel part of ref:datasets/transforms.py (RandomCrop, RandomTransformSE3_euler,
 * Resampler, RandomJitter, ShufflePoints) for many clouds in one launch each, after the host has drawn the random numbers
 * in the reference's order (csrc/modelnet.hip, pcrcg_amd/modelnet_prep.py).
 *
 * pcrcg_modelnet_crop -- RandomCrop.crop for C clouds.  pts [n_total, ld] f32, ld = 3 or 6 (xyz first); cloud c is rows
 *   off[c] .. off[c+1] (off [C+1] i32, on the device).  Per cloud: mode[c] (0 keep every row, 1 dist > 0, 2 percentile),
 *   dir [C, 3] f64 (the plane's normal), lo[c] and gamma[c] (the percentile's lower order statistic and its weight; read in
 *   mode 2 only).  kept [n_total] i32 receives, at rows off[c] .. off[c] + count[c], the kept rows' indices local to the
 *   cloud in ascending order (rows past the count are not written); count [C] i32 the number kept.
 *   Arithmetic contract (the file is compiled with -ffp-contract=off):
 *     centroid   the three columns added in f32 in row order, then divided by (float)n -- numpy's np.mean(axis=0) of a
 *                float32 array, bit for bit (a tree sum would round differently);
 *     dist       (f64(cx) * d0 + f64(cy) * d1) + f64(cz) * d2 with c = p - centroid in f32, nothing fused;
 *     threshold  mode 1: 0.  mode 2: numpy's 'linear' percentile of dist -- with a, b the lo-th and (lo+1)-th smallest
 *                distances (0-based), a + (b - a) * gamma, or b - (b - a) * (1 - gamma) when gamma >= 0.5; a itself when
 *                lo + 1 == n.  lo is clamped to 0 .. n - 1;
 *     mask       a row is kept iff dist > threshold, the literal comparison: rows that tie with the threshold are dropped,
 *                as numpy drops them (no rank cut);
 *     order      the compaction is stable.
 *   One workgroup per cloud with the distances resident in LDS; the order statistics come from a bitonic sort of a copy.  A
 *   workgroup holds PCRCG_MODELNET_CROP_MAX_ROWS rows (two float64 arrays of that length are 128 KiB of gfx950's 160 KiB);
 *   max_rows is the caller's statement of the longest cloud and sizes the LDS of the launch: max_rows above the capacity
 *   is rejected with PCRCG_EBADARG before anything is launched, and a cloud longer than max_rows gets count -1.
 *   count -1 also marks a cloud with a non-finite x, y or z, and a mode outside 0..2.  dir and gamma are the caller's: a
 *   non-finite one makes the distances or the threshold NaN, every comparison false and the count 0 (nothing else happens).  An offsets pair that does not describe a
 *   range inside the stack (negative, descending, past n_total) reads as an empty cloud: count 0.  No argument can cause
 *   an out-of-bounds access.  No workspace, no atomics, nothing allocated or synchronised.
 *
 * pcrcg_modelnet_assemble -- one output row per thread: out[i] = f32(f64(T . raw[kept[pick[i]]]) + noise[i]).
 *   raw [n_total, ld], in_off [C+1]: the input stack as above; kept / kept_count: pcrcg_modelnet_crop's outputs, or both
 *   NULL (every row kept).  The m_total output rows form K output clouds: rows out_off[k] .. out_off[k+1] (out_off [K+1])
 *   read input cloud out_cloud[k]; out_flags[k] bit 0: the cloud is moved by tf[k] ([K, 12] f32, a row-major [3, 4]), bit
 *   1: its rows receive noise ([m_total, 3] f64, in output order).  tf or noise may be NULL: the flag then does nothing.
 *   pick [m_total] i32 indexes the input cloud's kept list.  Arithmetic: xyz = ((x r0 + y r1) + z r2) + t in unfused f32;
 *   then f32(f64(v) + noise) per coordinate; normals (ld = 6) = (u r0 + v r1) + w r2, no translation, no noise; an
 *   untouched value is copied.  out [m_total, ld] f32.  A pick outside the kept list, a kept index outside its cloud, or a
 *   bad cloud index or offsets pair writes a row of NaN; a row that belongs to no output cloud is left alone.  No
 *   out-of-bounds access is possible through the device arrays. */
#define PCRCG_MODELNET_CROP_MAX_ROWS 8192
int pcrcg_modelnet_crop(const float* pts, int ld, int n_total, const int* off, int C, int max_rows, const int* mode,
                        const double* dir, const int* lo, const double* gamma, int* kept, int* count, void* stream);
int pcrcg_modelnet_assemble(const float* raw, int ld, int n_total, const int* in_off, int C, const int* kept,
                            const int* kept_count, const int* out_off, const int* out_cloud, const int* out_flags,
                            const float* tf, int K, const int* pick, const double* noise, int m_total, float* out,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PCRCG_H */
