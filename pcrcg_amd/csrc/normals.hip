// normals.hip -- surface normals of B ragged clouds on gfx950: what the point-to-plane ICP of icp.hip reads.
// ABI: include/pcrcg.h, section "Normal estimation"; DESIGN.md section 10 defines the algorithm and tests/normals_ref.py
// restates it in numpy.
//
// open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)), restated: one wavefront per point.
//   search  : hybrid_search.h (probe 27 cells, collect the supports with fp32 d2 < (float)r * (float)r, rank by (d2, index),
//             cut to max_nn on the way), with a list of 128 entries: up to 64 kept + 64 of the current step.
//   moments : lane k takes neighbour k's nine float64 terms (d, d d^T with d = q - p); a shuffle tree adds them.
//   normal  : lane 0 forms the covariance, runs the 3 x 3 Jacobi (smallsolve.h), orients the vector and stores it.
// No neighbour table goes to memory, and nothing is added by atomics: a row's bits depend on its cloud's points alone.
//
// Compiled with -ffp-contract=off (every operation rounds where the source says).
#include "common.h"
#include "hybrid_search.h"
#include "smallsolve.h"

namespace pcrcg {
namespace {

constexpr int kNrmWaves = 4;                      // points per workgroup
constexpr int kNrmCap = 128;                      // list entries per wavefront: up to 64 kept + 64 of the current step
constexpr int kNrmMaxNn = 64;                     // one neighbour per lane
constexpr int kNrmMaxBatch = 65535;               // clouds ride on a grid dimension

typedef HybridLds<kNrmWaves, kNrmCap> NrmLds;     // the search's lists (hybrid_search.h)

struct NrmArgs {
    const float* pts;
    const int* off;
    const double* viewpoints;   // [B, 3] or null
    double* normals;            // [n_total, 3]
    int* count;                 // [n_total] or null
    double* cov;                // [n_total, 6] or null
    float r2;
    int max_nn;
};

// grid (blocks of four rows, cloud)
__global__ void __launch_bounds__(kNrmWaves* kWave) k_estimate_normals(NrmArgs a, GridView g) {
    __shared__ NrmLds s;
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int b = blockIdx.y;
    const int i0 = a.off[b], n = a.off[b + 1] - i0;
    const int il = blockIdx.x * kNrmWaves + wave;
    if (il >= n) return;
    const long i = (long)i0 + il;
    const float px = a.pts[3 * i], py = a.pts[3 * i + 1], pz = a.pts[3 * i + 2];
    const HybridList<kNrmCap>& l = s.list[wave];
    int cur;
    const int k = hybrid_search(s, wave, lane, px, py, pz, g, b, a.r2, a.max_nn, &cur);          // k <= max_nn <= 64

    // lane e: neighbour e's terms about the query point
    double v[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) v[e] = 0.0;
    if (lane < k) {
        const float4 q = l.q[cur][lane];
        const double dx = (double)q.x - (double)px, dy = (double)q.y - (double)py, dz = (double)q.z - (double)pz;
        v[0] = dx; v[1] = dy; v[2] = dz;
        v[3] = dx * dx; v[4] = dx * dy; v[5] = dx * dz; v[6] = dy * dy; v[7] = dy * dz; v[8] = dz * dz;
    }
#pragma unroll
    for (int e = 0; e < 9; ++e)
#pragma unroll
        for (int sh = kWave / 2; sh >= 1; sh >>= 1) v[e] = v[e] + __shfl_down(v[e], sh, kWave);
    if (lane != 0) return;

    double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (k > 0) {
        const double kk = (double)k;
        const double mx = v[0] / kk, my = v[1] / kk, mz = v[2] / kk;
        C[0] = v[3] / kk - mx * mx; C[1] = v[4] / kk - mx * my; C[2] = v[5] / kk - mx * mz;
        C[3] = v[6] / kk - my * my; C[4] = v[7] / kk - my * mz; C[5] = v[8] / kk - mz * mz;
    }
    double nv[3] = {0.0, 0.0, 1.0};
    if (k >= 3 && smallest_eigenvector_sym3(C, nv)) {
        // towards the viewpoint; on the plane through it, the first non-zero component positive
        double vx = 0.0, vy = 0.0, vz = 0.0;
        if (a.viewpoints) { vx = a.viewpoints[3 * b]; vy = a.viewpoints[3 * b + 1]; vz = a.viewpoints[3 * b + 2]; }
        const double dot = (nv[0] * (vx - (double)px) + nv[1] * (vy - (double)py)) + nv[2] * (vz - (double)pz);
        const double lead = nv[0] != 0.0 ? nv[0] : (nv[1] != 0.0 ? nv[1] : nv[2]);
        if (dot < 0.0 || (dot == 0.0 && lead < 0.0)) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
    }
    double* o = a.normals + 3 * i;
    o[0] = nv[0]; o[1] = nv[1]; o[2] = nv[2];
    if (a.count) a.count[i] = k;
    if (a.cov)
        for (int e = 0; e < 6; ++e) a.cov[6 * i + e] = C[e];
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_estimate_normals_ws_bytes(int B, int n_total) {
    if (B < 1 || B > kNrmMaxBatch || n_total < 0) return 0;
    return 256;                                   // nothing is staged today; a non-zero size keeps one calling pattern
}

int pcrcg_estimate_normals_batch(const float* pts, const int* off, int n_total, int n_max, const void* grid, int B, double radius,
                                 int max_nn, const double* viewpoints, double* normals, int* count, double* cov, void* ws,
                                 size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(off && grid && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kNrmMaxBatch);
    PCRCG_CHECK_ARG(n_total >= 0 && n_max >= 0 && n_max <= n_total);
    PCRCG_CHECK_ARG(n_total == 0 || (pts && normals));
    PCRCG_CHECK_ARG(radius > 0.0 && radius < 1e18);                         // (false for a NaN)
    PCRCG_CHECK_ARG(max_nn >= 1 && max_nn <= kNrmMaxNn);
    Carver cv(ws, ws_bytes);
    cv.take<char>(pcrcg_estimate_normals_ws_bytes(B, n_total));
    PCRCG_CHECK_WS(cv);
    if (n_max == 0) return PCRCG_OK;
    bool ok;
    GridView g = grid_view(const_cast<void*>(grid), grid_bytes(n_total, B), n_total, B, &ok);
    NrmArgs a;
    a.pts = pts; a.off = off; a.viewpoints = viewpoints;
    a.normals = normals; a.count = count; a.cov = cov;
    a.r2 = (float)radius * (float)radius;
    a.max_nn = max_nn;
    hipLaunchKernelGGL(k_estimate_normals, dim3((n_max + kNrmWaves - 1) / kNrmWaves, B), dim3(kNrmWaves * kWave), 0,
                       as_stream(stream), a, g);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
