// colored.hip -- colour gradients of B ragged target clouds on gfx950: what the colored ICP of icp.hip (EST = 3) reads.
// ABI: include/pcrcg.h, section "Colored ICP"; DESIGN.md section 24 explains the algorithm and tests/colored_icp_ref.py
// restates it in numpy.
//
// open3d 0.10's InitializePointCloudForColoredICP (Park, Zhou, Koltun, ICCV 2017), restated: one wavefront per point.
//   search   : hybrid_search.h with a list of 128 entries (up to 64 kept + 64 of the current step), as normals.hip.
//   rows     : lane e in 1 .. k - 1 projects neighbour e onto the point's tangent plane and forms the nine products of its
//              row of the least-squares fit I(a) - I(k) = g . (proj(a) - p) (colored_terms.h); the neighbour's intensity is
//              gathered by the index in q.w; a shuffle tree adds the rows.
//   gradient : lane 0 adds the last row (k - 1) n, solves the 3 x 3 normal equations by the pivoted LDL^T of smallsolve.h and
//              stores the point's packed record (n [3], g [3], I, 0): one aligned 64-byte load per correspondence later.
// A list shorter than 4, or a refused solve, gives g = 0.  No neighbour table goes to memory, and nothing is added by
// atomics: a row's bits depend on its cloud's points, normals and intensities alone.
//
// Compiled with -ffp-contract=off (every operation rounds where the source says).
#include "colored_terms.h"
#include "common.h"
#include "hybrid_search.h"
#include "smallsolve.h"

namespace pcrcg {
namespace {

constexpr int kColWaves = 4;                      // points per workgroup
constexpr int kColCap = 128;                      // list entries per wavefront: up to 64 kept + 64 of the current step
constexpr int kColMaxNn = 64;                     // one neighbour per lane
constexpr int kColMinNn = 4;                      // open3d: a shorter list gives no gradient
constexpr int kColMaxBatch = 65535;               // clouds ride on a grid dimension

typedef HybridLds<kColWaves, kColCap> ColLds;

struct ColArgs {
    const float* pts;
    const int* off;
    const double* normals;      // [n_total, 3]
    const double* intensity;    // [n_total]
    double* rec;                // [n_total, 8]
    int* count;                 // [n_total] or null
    double* sums;               // [n_total, 9] or null
    float r2;
    int max_nn;
};

// grid (blocks of four rows, cloud)
__global__ void __launch_bounds__(kColWaves* kWave) k_color_gradients(ColArgs a, GridView g) {
    __shared__ ColLds s;
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int b = blockIdx.y;
    const int i0 = a.off[b], n = a.off[b + 1] - i0;
    const int il = blockIdx.x * kColWaves + wave;
    if (il >= n) return;
    const long i = (long)i0 + il;
    const float px = a.pts[3 * i], py = a.pts[3 * i + 1], pz = a.pts[3 * i + 2];
    const HybridList<kColCap>& l = s.list[wave];
    int cur;
    const int k = hybrid_search(s, wave, lane, px, py, pz, g, b, a.r2, a.max_nn, &cur);          // k <= max_nn <= 64

    const double vt[3] = {(double)px, (double)py, (double)pz};
    const double nt[3] = {a.normals[3 * i], a.normals[3 * i + 1], a.normals[3 * i + 2]};
    const double Ik = a.intensity[i];
    // lane e: the row of entry e; entry 0 is dropped whichever point it is
    double v[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) v[e] = 0.0;
    if (k >= kColMinNn && lane >= 1 && lane < k) {
        const float4 q = l.q[cur][lane];
        const double pa[3] = {(double)q.x, (double)q.y, (double)q.z};
        colored_gradient_row(vt, nt, pa, a.intensity[__float_as_int(q.w)], Ik, v);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e)
#pragma unroll
        for (int sh = kWave / 2; sh >= 1; sh >>= 1) v[e] = v[e] + __shfl_down(v[e], sh, kWave);
    if (lane != 0) return;

    double gr[3] = {0.0, 0.0, 0.0};
    if (k >= kColMinNn) {
        colored_gradient_last_row(nt, k, v);
        double x[3];
        if (solve_ldlt3(v, v + 6, x)) { gr[0] = x[0]; gr[1] = x[1]; gr[2] = x[2]; }
    }
    double* o = a.rec + 8 * i;
    o[0] = nt[0]; o[1] = nt[1]; o[2] = nt[2];
    o[3] = gr[0]; o[4] = gr[1]; o[5] = gr[2];
    o[6] = Ik;
    o[7] = 0.0;
    if (a.count) a.count[i] = k;
    if (a.sums)
        for (int e = 0; e < 9; ++e) a.sums[9 * i + e] = v[e];
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_color_gradients_ws_bytes(int B, int n_total) {
    if (B < 1 || B > kColMaxBatch || n_total < 0) return 0;
    return 256;                                   // nothing is staged: the lists live in LDS; one calling pattern
}

int pcrcg_color_gradients_batch(const float* pts, const int* off, int n_total, int n_max, const void* grid, int B, double radius,
                                int max_nn, const double* normals, const double* intensity, double* rec, int* count, double* sums,
                                void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(off && grid && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kColMaxBatch);
    PCRCG_CHECK_ARG(n_total >= 0 && n_max >= 0 && n_max <= n_total);
    PCRCG_CHECK_ARG(n_total == 0 || (pts && normals && intensity && rec));
    PCRCG_CHECK_ARG(radius > 0.0 && radius < 1e18);                         // (false for a NaN)
    PCRCG_CHECK_ARG(max_nn >= 1 && max_nn <= kColMaxNn);
    Carver cv(ws, ws_bytes);
    cv.take<char>(pcrcg_color_gradients_ws_bytes(B, n_total));
    PCRCG_CHECK_WS(cv);
    if (n_max == 0) return PCRCG_OK;
    bool ok;
    GridView g = grid_view(const_cast<void*>(grid), grid_bytes(n_total, B), n_total, B, &ok);
    ColArgs a;
    a.pts = pts; a.off = off; a.normals = normals; a.intensity = intensity;
    a.rec = rec; a.count = count; a.sums = sums;
    a.r2 = (float)radius * (float)radius;
    a.max_nn = max_nn;
    hipLaunchKernelGGL(k_color_gradients, dim3((n_max + kColWaves - 1) / kColWaves, B), dim3(kColWaves * kWave), 0,
                       as_stream(stream), a, g);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
