// fgr.hip -- fast global registration on gfx950: B pairs side by side, one workgroup per pair, one launch.
// ABI: include/pcrcg.h, section "Fast global registration" (the definition; DESIGN.md section 22 has the reasoning and the
// measurements, tests/fgr_ref.py restates it in numpy float64).
//
// After Zhou, Park, Koltun, "Fast Global Registration" (ECCV 2016) and open3d's
// registration_fast_based_on_feature_matching, with the departures the header lists.  Per pair, from a correspondence
// list (pcrcg_mutual_match_batch's, pcrcg_feature_match_batch's or the caller's own):
//
//   tuples    : trials t = 0 .. 100 P - 1 in rounds of one per thread; a trial draws three rows of the list by splitmix64 and
//               passes when the three edge lengths agree within tuple_scale on both sides (float64).  A block scan ranks a
//               round's passes, so the first maximum_tuple_count passing trials are accepted in trial order whatever the
//               schedule.  Their rows, three per trial, are the entry list E.
//   frame     : the centroids of E's source and target points and D^2, the largest squared distance of a centred point.
//   iterations: iteration_number Gauss-Newton steps on sum l |R p + t - q|^2 with the Geman-McClure weight
//               l = (mu / (|r|^2 + mu))^2, mu graduated from D^2 towards delta^2.  The 27 float64 sums of a step are added
//               per thread over its entries in ascending order, then by a shuffle tree inside each wavefront, then the eight
//               wavefronts one after the other: a fixed order, no floating-point atomics.  One lane solves the 6 x 6 system
//               (smallsolve.h, as icp.hip's point-to-plane update) and hands T to the others through LDS.
//
// E's points (24 bytes per entry) are loaded once: into LDS when 3 maximum_tuple_count entries fit 96 KB, otherwise into the
// workspace (L2).  Every loop has a bound the host knows: 100 P <= 100 n_b trials, iteration_number steps.  A workgroup never
// waits for another.
//
// Compiled with -ffp-contract=off: every float64 operation rounds where the source says.
#include "block_scan.h"
#include "common.h"
#include "smallsolve.h"
#include "splitmix.h"

namespace pcrcg {
namespace {

typedef unsigned long long u64;

constexpr int kFgrThreads = 512;
constexpr int kFgrWaves = kFgrThreads / kWave;
constexpr int kFgrTerms = 27;                    // the upper triangle of A (21), then g (6)
constexpr int kFgrMaxBatch = 65535;              // pairs ride on a grid dimension
constexpr int kFgrMaxTuples = 4096;
constexpr int kFgrMaxIteration = 1 << 16;
constexpr int kFgrMinEntries = 10;               // fewer entries than this: the identity
constexpr int kFgrLdsEntries = 4096;             // 3 maximum_tuple_count up to this: E's points live in LDS (96 KB)

struct FgrArgs {
    const float* src; const int* src_off;
    const float* tgt; const int* tgt_off;
    const int* corr; const int* k;
    const u64* seeds;
    double delta2, division_factor, tuple_scale;
    int decrease_mu, iteration_number, max_tuples;
    double* out_t; double* out_stats;
    int* ws_e;            // [B, 3 max_tuples, 2]
    float* ws_pts;        // [B, 3 max_tuples, 6]
    pcrcg_fgr_trace tr;
};

__device__ inline double edge_length(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// v[0 .. N-1] of every thread -> s_tot[0 .. N-1]: the wavefront's shuffle tree, then the wavefronts in order.  Two barriers;
// every thread of the workgroup calls it.
template <int N>
__device__ inline void block_sum(double* v, double (*s_part)[kFgrTerms], double* s_tot) {
#pragma unroll
    for (int e = 0; e < N; ++e)
#pragma unroll
        for (int sh = kWave / 2; sh >= 1; sh >>= 1) v[e] = v[e] + __shfl_down(v[e], sh, kWave);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < N; ++e) s_part[wave][e] = v[e];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double s = s_part[0][threadIdx.x];
        for (int w = 1; w < kFgrWaves; ++w) s = s + s_part[w][threadIdx.x];
        s_tot[threadIdx.x] = s;
    }
    __syncthreads();
}

__device__ inline void fgr_write(const FgrArgs& a, int b, const double* R, const double* t, double P, double tuples, double trials,
                                 double updates, double mu, double share) {
    double* o = a.out_t + 16 * (long)b;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[4 * r + c] = R[3 * r + c];
        o[4 * r + 3] = t[r];
    }
    o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
    double* s = a.out_stats + 6 * (long)b;
    s[0] = P; s[1] = tuples; s[2] = trials; s[3] = updates; s[4] = mu; s[5] = share;
}

__global__ void __launch_bounds__(kFgrThreads) k_fgr(FgrArgs a, int use_lds) {
    extern __shared__ __attribute__((aligned(16))) float s_pts[];
    __shared__ double s_part[kFgrWaves][kFgrTerms];
    __shared__ double s_tot[kFgrTerms];
    __shared__ double s_T[12];
    __shared__ double s_mu;
    __shared__ long long s_last;
    __shared__ int s_scan[kFgrWaves];
    __shared__ int s_stop, s_updates;
    const int b = blockIdx.x, tid = threadIdx.x;
    const u64 seed = a.seeds[b];
    if (seed >= (1ull << 24)) {
        if (tid < 16) a.out_t[16 * (long)b + tid] = __builtin_nan("");
        if (tid < 6) a.out_stats[6 * (long)b + tid] = __builtin_nan("");
        return;
    }
    const int i0 = a.src_off[b], n = a.src_off[b + 1] - i0;
    const int j0 = a.tgt_off[b], m = a.tgt_off[b + 1] - j0;
    int P = a.k[b];
    P = P < 0 ? 0 : P;
    P = P > n ? n : P;
    if (n <= 0 || m <= 0) P = 0;              // nothing to index
    const float* src = a.src + 3 * (long)i0;
    const float* tgt = a.tgt + 3 * (long)j0;
    const int* corr = a.corr + 2 * (long)i0;
    const int cap = a.max_tuples;
    int* E = a.ws_e + 2 * (long)b * 3 * cap;
    float* pts = use_lds ? s_pts : a.ws_pts + 6 * (long)b * 3 * cap;
    const double identity_R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, zero_t[3] = {0.0, 0.0, 0.0};

    // ---- tuple stage ----
    int nE = 0, accepted = 0;
    long long trials_used = 0;
    if (a.tuple_scale == 0.0) {
        nE = P < 3 * cap ? P : 3 * cap;
        for (int e = tid; e < nE; e += kFgrThreads) { E[2 * e] = corr[2 * e]; E[2 * e + 1] = corr[2 * e + 1]; }
    } else {
        const long long total = 100ll * (long long)P;
        trials_used = total;
        for (long long t0 = 0; t0 < total && accepted < cap; t0 += kFgrThreads) {
            const long long t = t0 + tid;
            bool pass = false;
            int rows[3] = {0, 0, 0};
            if (t < total) {
                double p[3][3], q[3][3];
                for (int s = 0; s < 3; ++s) {
                    const u64 r = splitmix64((seed << 40) + 4ull * (u64)t + (u64)s);
                    rows[s] = (int)(((r >> 32) * (u64)P) >> 32);
                    const int i = corr[2 * rows[s]], j = corr[2 * rows[s] + 1];
                    for (int c = 0; c < 3; ++c) { p[s][c] = (double)src[3 * (long)i + c]; q[s][c] = (double)tgt[3 * (long)j + c]; }
                }
                pass = true;
                for (int s = 0; s < 3; ++s) {
                    const int s2 = s == 2 ? 0 : s + 1;
                    const double li = edge_length(p[s], p[s2]), lj = edge_length(q[s], q[s2]);
                    pass = pass && li * a.tuple_scale < lj && lj * a.tuple_scale < li;
                }
            }
            int round_total;
            const int rank = block_excl_scan_i32<kFgrThreads>(pass ? 1 : 0, &round_total, s_scan);
            const int slot = accepted + rank;
            if (pass && slot < cap) {
                for (int s = 0; s < 3; ++s) {
                    E[2 * (3 * slot + s)] = corr[2 * rows[s]];
                    E[2 * (3 * slot + s) + 1] = corr[2 * rows[s] + 1];
                }
                if (a.tr.trials) a.tr.trials[(long)b * cap + slot] = t;
                if (slot == cap - 1) s_last = t + 1;
            }
            accepted = accepted + round_total < cap ? accepted + round_total : cap;
        }
        __syncthreads();
        if (accepted == cap) trials_used = s_last;
        nE = 3 * accepted;
    }
    __syncthreads();
    // E's points, loaded once; the trace of E
    for (int e = tid; e < nE; e += kFgrThreads) {
        const int i = E[2 * e], j = E[2 * e + 1];
        for (int c = 0; c < 3; ++c) { pts[6 * e + c] = src[3 * (long)i + c]; pts[6 * e + 3 + c] = tgt[3 * (long)j + c]; }
        if (a.tr.entries) { a.tr.entries[2 * ((long)b * 3 * cap + e)] = i; a.tr.entries[2 * ((long)b * 3 * cap + e) + 1] = j; }
    }
    __syncthreads();
    if (nE < kFgrMinEntries) {
        if (tid == 0) fgr_write(a, b, identity_R, zero_t, (double)P, (double)accepted, (double)trials_used, 0.0, 0.0, 0.0);
        return;
    }

    // ---- frame ----
    double v[kFgrTerms];
#pragma unroll
    for (int e = 0; e < 6; ++e) v[e] = 0.0;
    for (int e = tid; e < nE; e += kFgrThreads)
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] = v[c] + (double)pts[6 * e + c];
    block_sum<6>(v, s_part, s_tot);
    double cs[3], ct[3];
    for (int c = 0; c < 3; ++c) { cs[c] = s_tot[c] / (double)nE; ct[c] = s_tot[3 + c] / (double)nE; }
    double d2 = 0.0;
    for (int e = tid; e < nE; e += kFgrThreads) {
        const double px = (double)pts[6 * e] - cs[0], py = (double)pts[6 * e + 1] - cs[1], pz = (double)pts[6 * e + 2] - cs[2];
        const double qx = (double)pts[6 * e + 3] - ct[0], qy = (double)pts[6 * e + 4] - ct[1], qz = (double)pts[6 * e + 5] - ct[2];
        d2 = fmax(d2, fmax((px * px + py * py) + pz * pz, (qx * qx + qy * qy) + qz * qz));
    }
    for (int sh = kWave / 2; sh >= 1; sh >>= 1) d2 = fmax(d2, __shfl_down(d2, sh, kWave));
    __syncthreads();                              // (s_part: the centroid sums have been read)
    if ((tid & (kWave - 1)) == 0) s_part[tid / kWave][0] = d2;
    __syncthreads();
    double D2 = s_part[0][0];
    for (int w = 1; w < kFgrWaves; ++w) D2 = fmax(D2, s_part[w][0]);
    if (tid == 0 && a.tr.frame) {
        double* f = a.tr.frame + 7 * (long)b;
        for (int c = 0; c < 3; ++c) { f[c] = cs[c]; f[3 + c] = ct[c]; }
        f[6] = D2;
    }
    if (!(D2 > 0.0) || !(D2 <= 1.79769313486231570815e308)) {
        if (tid == 0) fgr_write(a, b, identity_R, zero_t, (double)P, (double)accepted, (double)trials_used, 0.0, D2, 0.0);
        return;
    }

    // ---- iterations ----
    if (tid == 0) {
        for (int e = 0; e < 12; ++e) s_T[e] = (e == 0 || e == 5 || e == 10) ? 1.0 : 0.0;    // rows of [R | t]
        s_mu = D2;
        s_stop = 0;
        s_updates = 0;
    }
    __syncthreads();
    for (int it = 0; it < a.iteration_number; ++it) {
        double T[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = s_T[e];
        const double mu = s_mu;
#pragma unroll
        for (int e = 0; e < kFgrTerms; ++e) v[e] = 0.0;
        for (int e = tid; e < nE; e += kFgrThreads) {
            const double x = (double)pts[6 * e] - cs[0], y = (double)pts[6 * e + 1] - cs[1], z = (double)pts[6 * e + 2] - cs[2];
            const double px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
            const double py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
            const double pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
            const double rx = px - ((double)pts[6 * e + 3] - ct[0]);
            const double ry = py - ((double)pts[6 * e + 4] - ct[1]);
            const double rz = pz - ((double)pts[6 * e + 5] - ct[2]);
            const double w = mu / (((rx * rx + ry * ry) + rz * rz) + mu);
            const double l = w * w;
            // J_x = (0, pz, -py, 1, 0, 0), J_y = (-pz, 0, px, 0, 1, 0), J_z = (py, -px, 0, 0, 0, 1): the upper triangle of
            // J_x J_x^T + J_y J_y^T + J_z J_z^T row by row, then J_x r_x + J_y r_y + J_z r_z
            v[0] = v[0] + l * (pz * pz + py * py);
            v[1] = v[1] + l * (-(px * py));
            v[2] = v[2] + l * (-(px * pz));
            v[4] = v[4] + l * (-pz);
            v[5] = v[5] + l * py;
            v[6] = v[6] + l * (pz * pz + px * px);
            v[7] = v[7] + l * (-(py * pz));
            v[8] = v[8] + l * pz;
            v[10] = v[10] + l * (-px);
            v[11] = v[11] + l * (py * py + px * px);
            v[12] = v[12] + l * (-py);
            v[13] = v[13] + l * px;
            v[15] = v[15] + l;
            v[21] = v[21] + l * (py * rz - pz * ry);
            v[22] = v[22] + l * (pz * rx - px * rz);
            v[23] = v[23] + l * (px * ry - py * rx);
            v[24] = v[24] + l * rx;
            v[25] = v[25] + l * ry;
            v[26] = v[26] + l * rz;
        }
        v[18] = v[15];                      // A44 = A55 = A33 = sum l; A03, A14, A25, A34, A35, A45 stay 0
        v[20] = v[15];
#pragma unroll
        for (int e = 21; e < kFgrTerms; ++e) v[e] = -v[e];   // g = -sum l J r
        block_sum<kFgrTerms>(v, s_part, s_tot);
        if (tid == 0) {
            const long slot = (long)b * a.iteration_number + it;
            if (a.tr.transforms) {
                double* o = a.tr.transforms + 16 * slot;
                for (int e = 0; e < 12; ++e) o[e] = T[e];
                o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
            }
            if (a.tr.mu) a.tr.mu[slot] = mu;
            if (a.tr.sums27)
                for (int e = 0; e < kFgrTerms; ++e) a.tr.sums27[kFgrTerms * slot + e] = s_tot[e];
            double x[6];
            if (!solve_ldlt6(s_tot, s_tot + 21, x)) {
                s_stop = 1;
            } else {
                // delta = Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5), as icp.hip's point-to-plane update; T <- delta T
                const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
                const double R[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                                     sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                                     -sb,     cb * sa,                cb * ca};
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 4; ++c) {
                        const double u = (R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c]) + R[3 * r + 2] * T[8 + c];
                        s_T[4 * r + c] = c == 3 ? u + x[3 + r] : u;
                    }
                s_updates = s_updates + 1;
                if (a.decrease_mu && it % 4 == 0 && mu > a.delta2) s_mu = mu / a.division_factor;
            }
        }
        __syncthreads();
        if (s_stop) break;
    }

    // ---- output ----
    double T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = s_T[e];
    int inl = 0;
    for (int e = tid; e < nE; e += kFgrThreads) {
        const double x = (double)pts[6 * e] - cs[0], y = (double)pts[6 * e + 1] - cs[1], z = (double)pts[6 * e + 2] - cs[2];
        const double rx = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - ((double)pts[6 * e + 3] - ct[0]);
        const double ry = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - ((double)pts[6 * e + 4] - ct[1]);
        const double rz = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - ((double)pts[6 * e + 5] - ct[2]);
        if ((rx * rx + ry * ry) + rz * rz < a.delta2) ++inl;
    }
    int inliers;
    block_excl_scan_i32<kFgrThreads>(inl, &inliers, s_scan);
    if (tid == 0) {
        double R[9], t[3];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R[3 * r + c] = T[4 * r + c];
            t[r] = (T[4 * r + 3] - ((T[4 * r] * cs[0] + T[4 * r + 1] * cs[1]) + T[4 * r + 2] * cs[2])) + ct[r];
        }
        fgr_write(a, b, R, t, (double)P, (double)accepted, (double)trials_used, (double)s_updates, s_mu,
                  (double)inliers / (double)nE);
    }
}

struct FgrWs {
    int* e;
    float* pts;
};

FgrWs carve_fgr(Carver& cv, int B, int max_tuples) {
    FgrWs w;
    const size_t entries = (size_t)B * 3 * (size_t)max_tuples;
    w.e = cv.take<int>(entries * 2);
    w.pts = cv.take<float>(entries * 6);
    return w;
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_fgr_batch_ws_bytes(int B, int n_total, int maximum_tuple_count, int iteration_number) {
    if (B < 1 || B > kFgrMaxBatch || n_total < 0 || maximum_tuple_count < 1 || maximum_tuple_count > kFgrMaxTuples ||
        iteration_number < 1 || iteration_number > kFgrMaxIteration)
        return 0;
    Carver cv(nullptr, 0);
    carve_fgr(cv, B, maximum_tuple_count);
    return cv.off;
}

int pcrcg_fgr_batch(const float* src, const int* src_off, const float* tgt, const int* tgt_off, const int* corr, const int* k, int B,
                    double maximum_correspondence_distance, double division_factor, int decrease_mu, int iteration_number,
                    double tuple_scale, int maximum_tuple_count, const uint64_t* seeds, double* out_transform, double* out_stats,
                    const pcrcg_fgr_trace* trace, void* ws, size_t ws_bytes, void* stream) {
    PCRCG_CHECK_ARG(src && src_off && tgt && tgt_off && corr && k && seeds && out_transform && out_stats && ws);
    PCRCG_CHECK_ARG(B >= 1 && B <= kFgrMaxBatch);
    PCRCG_CHECK_ARG(maximum_correspondence_distance > 0.0 && maximum_correspondence_distance <= 1.79769313486231570815e308);   // (false for a NaN)
    PCRCG_CHECK_ARG(division_factor > 1.0 && division_factor <= 1.79769313486231570815e308);
    PCRCG_CHECK_ARG(decrease_mu == 0 || decrease_mu == 1);
    PCRCG_CHECK_ARG(iteration_number >= 1 && iteration_number <= kFgrMaxIteration);
    PCRCG_CHECK_ARG(tuple_scale >= 0.0 && tuple_scale <= 1.0);
    PCRCG_CHECK_ARG(maximum_tuple_count >= 1 && maximum_tuple_count <= kFgrMaxTuples);
    Carver cv(ws, ws_bytes);
    FgrWs w = carve_fgr(cv, B, maximum_tuple_count);
    PCRCG_CHECK_WS(cv);
    FgrArgs a;
    a.src = src; a.src_off = src_off; a.tgt = tgt; a.tgt_off = tgt_off; a.corr = corr; a.k = k;
    a.seeds = reinterpret_cast<const u64*>(seeds);
    a.delta2 = maximum_correspondence_distance * maximum_correspondence_distance;
    a.division_factor = division_factor; a.tuple_scale = tuple_scale;
    a.decrease_mu = decrease_mu; a.iteration_number = iteration_number; a.max_tuples = maximum_tuple_count;
    a.out_t = out_transform; a.out_stats = out_stats;
    a.ws_e = w.e; a.ws_pts = w.pts;
    a.tr = pcrcg_fgr_trace{};
    if (trace) a.tr = *trace;
    const int entries = 3 * maximum_tuple_count;
    const int use_lds = entries <= kFgrLdsEntries ? 1 : 0;
    const size_t lds = use_lds ? (size_t)entries * 6 * sizeof(float) : 0;
    PCRCG_GRANT_LDS(k_fgr);
    hipLaunchKernelGGL(k_fgr, dim3(B), dim3(kFgrThreads), lds, as_stream(stream), a, use_lds);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}  // extern "C"
