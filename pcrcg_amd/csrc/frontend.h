// frontend.h -- what the front-end files (grid_subsample.hip, radius.hip, tieorder.hip) offer the pyramid builder
// (pyramid.hip) and one another beyond the C ABI of pcrcg.h, declared here and nowhere else.
#pragma once
#include "common.h"

namespace pcrcg {

// grid_subsample.hip: pcrcg_grid_subsample_batch with the number of points given as a host-side BOUND (the cloud
// lengths on the device say how many there are) and room for out_cap output rows (more: *overflow = 1, output cut)
int grid_subsample_bound(const float* pts, int n_bound, const int* len, int nb, float dl, int max_p, float* out_pts,
                         int* out_len, int* out_m, int out_cap, int* overflow, void* ws, size_t ws_bytes, hipStream_t stream);

// tieorder.hip: pcrcg_kdforest_build over clouds that are LEVELS of per_level clouds each, level l's rows starting at row
// level_base[l] of sup (per_level = 0: one contiguous stack, the public entry point)
int kdforest_build_levels(const float* sup, int ns, const int* slen, int nb, int per_level, const int* level_base, void* forest,
                          size_t forest_bytes, hipStream_t stream);

// radius.hip: one radius search -- every list of up to `cols` neighbours of nq queries among ns supports.  The fields are
// the arguments of pcrcg_radius_query_groups / pcrcg_radius_query_cells (include/pcrcg.h says what each holds).
struct RadiusSearch {
    const float* q; int nq; const int* qlen;          // queries, their count (or a bound on it) and cloud lengths
    const void* qgrid;                                // a cell grid over the QUERIES: the cell kernel walks it; nullptr: per-query
    const void* sgrid; int ns; const int* slen;       // the supports' cell grid, their count and cloud lengths
    int nb, group; float radius; int cols;
    int64_t* idx; int* count; int* max_count; int* status; int* tie_rows; int* tie_count;
};
// both: the first kernel (cell-cooperative with a query grid, else per-query) and the per-query redo kernel behind it: what
// the public entries run.  first: the first kernel only; it marks the rows it cannot finish -- more hits than it stages
// (their true length goes to max_count), or, in the cell kernel, a cell whose neighbourhood does not fit LDS (status bit
// kRadiusRedoStatus announces both) -- and a caller that reads max_count and status anyway (the pyramid builder) launches
// redo, the per-query redo kernel alone, for the searches that need it: normally none.  It clears the status bit.
enum class RadiusPass { both, first, redo };
int radius_search(const RadiusSearch& s, RadiusPass pass, hipStream_t st);
int radius_fast_cap();
constexpr int kRadiusRedoStatus = 4;

}  // namespace pcrcg
