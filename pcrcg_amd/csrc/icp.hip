// icp.hip -- batched point-to-point ICP on gfx950: the local refinement after RANSAC (register.hip).
// ABI: include/pcrcg.h, section "ICP refinement"; DESIGN.md section 10 defines the algorithm and tests/icp_ref.py restates
// it in numpy.
//
// open3d 0.10's RegistrationICP with TransformationEstimationPointToPoint(false), restated for B ragged pairs:
//
//   evaluate : grid (row blocks, pair), one thread per source point.  T (float64, per pair, on the device) is rounded to
//              fp32, the point moved with the unfused fp32 arithmetic of RANSAC's evaluation and its nearest target looked
//              up in the pair's cell grid (27 cells), minimising over (d2, target index); a correspondence iff
//              d2 < (float)(d^2).  In the same pass every workgroup reduces, in a fixed order (wavefront shuffles, then its
//              eight wavefronts one after the other), the count and 16 float64 sums of its correspondences: d2, the moved
//              point p, its target q, and p q^T.
//   update   : one wavefront per pair adds the workgroups' partial sums in workgroup order, takes fitness and rmse,
//              applies the convergence test, fits delta (kabsch.h, the device function of RANSAC's hypotheses) and sets
//              T <- delta T in float64 -- or finishes the pair: writes its outputs and sets its `done` word.
//
// pcrcg_icp_batch_ex adds TransformationEstimationPointToPlane as a second estimator (template argument EST = 1 of the two
// kernels; EST = 0 is the code above, bit for bit): the evaluation is the same, its sums are d2, the upper triangle of
// sum J J^T and -sum J r with r = (p - q) . n, J = [p x n, n] from the targets' normals (normals.hip), and the update solves
// the 6 x 6 system by a pivoted LDL^T (smallsolve.h) and applies Rz Ry Rx | t of the solution.
//
// pcrcg_gicp_batch adds Generalized ICP as a third (EST = 2): the same evaluation again; every correspondence gathers the
// covariances of its two points, W = (C_t + R C_s R^T)^-1 and the 27 terms of J0^T W J0 and -J0^T W d come from gicp_terms.h,
// and the update is point-to-plane's solve and delta.  k_cov_from_normals builds such covariances from normals.
//
// pcrcg_colored_icp_batch adds colored ICP as a fourth (EST = 3): the same evaluation; every correspondence loads its target's
// packed record (normal, colour gradient, intensity: colored.hip) and its source's intensity, the 27 terms of the joint
// colour / geometry objective come from colored_terms.h, and the update is point-to-plane's solve and delta again.
//
// pcrcg_icp_plane_robust_batch and pcrcg_colored_icp_robust_batch put a robust loss kernel (robust_kernel.h: open3d's
// RobustKernel, a kind and a scale, uniform over the call) on EST = 1 and EST = 3: a second instantiation of the evaluation
// (ROBUST) multiplies every correspondence's terms with the weight of its residual where they are formed -- plane_terms_robust,
// colored_terms_robust.  Everything else is the plain estimator's: the search, the count, the d2 sum, the reductions, and
// k_icp_update<1> / <3>, which see only sums.
//
// Host side: every extern "C" entry fills one IcpCall -- the arguments all entries share, its estimator, and that
// estimator's own inputs by name -- and hands it to icp_run, the one place for the argument rules, the workspace carve, the
// fill of the kernels' IcpArgs and the dispatch to icp_enqueue<EST>.  A further estimator is one more entry that fills an
// IcpCall, its fields there and in IcpArgs (appended: the member order is the kernels' argument layout), one case in each of
// icp_run's two switches, and one `if constexpr` branch in each kernel.
//
// All max_iteration + 1 evaluations are enqueued ahead; the host reads nothing in between.  The workgroups of a pair whose
// `done` word is set leave at once.  No floating-point atomics: a pair's bits depend on its own points and T_0 alone.
//
// Compiled with -ffp-contract=off (every operation rounds where the source says).
#include "cellgrid.h"
#include "colored_terms.h"
#include "common.h"
#include "gicp_terms.h"
#include "kabsch.h"
#include "robust_kernel.h"
#include "smallsolve.h"

namespace pcrcg {
namespace {

constexpr int kIcpThreads = 512;                  // evaluation workgroup: 512 consecutive source rows of one pair
constexpr int kIcpWaves = kIcpThreads / kWave;
constexpr int kIcpTerms = 16;                     // sum d2 | sum p [3] | sum q [3] | sum p q^T [9]
constexpr int kIcpPlaneTerms = 28;                // sum d2 | sum J J^T, upper triangle [21] | -sum J r [6]; EST 2: J0^T W J0 | -J0^T W d
// EST 0: point-to-point, 1: point-to-plane, 2: generalized, 3: colored
template <int EST> constexpr int icp_terms() { return EST == 0 ? kIcpTerms : kIcpPlaneTerms; }
constexpr int kEstPoint = 0, kEstPlane = 1;       // EST of pcrcg_icp_batch; pcrcg_icp_batch_ex takes either
constexpr int kEstGeneralized = 2;                // EST of pcrcg_gicp_batch
constexpr int kEstColored = 3;                    // EST of pcrcg_colored_icp_batch
constexpr int kIcpMaxIteration = 1 << 16;
constexpr int kIcpMaxBatch = 65535;               // pairs ride on a grid dimension

struct IcpPair {          // the loop's state of one pair
    double T[16];         // T_k, row-major
    double fitness, rmse; // of Evaluate(T_k-1)
    int done;
    int pad;
};

struct IcpArgs {
    const float* src;
    const int* src_off;
    const int* tgt_off;
    const double* init;   // [B, 16] or null (identity)
    IcpPair* state;       // [B]
    int* p_cnt;           // [slots]      the workgroups' partial counts ...
    double* p_sum;        // [slots, 16 or 28]  ... and sums; pair p's workgroups start at slot src_off[p] / 512 + p
    double* out_t;        // [B, 16]
    double* out_stats;    // [B, 4]
    double* tr_t;         // [B, max_iteration + 1, 16] or null
    int* tr_counts;       // [B, max_iteration + 1] or null
    double* tr_sums;      // [B, max_iteration + 1] or null
    int* tr_corr;         // [max_iteration + 1, n_total] or null
    const double* tgt_nrm;// [m_total, 3] point-to-plane: the targets' normals
    double* tr_sums27;    // [B, max_iteration + 1, 27] or null (point-to-plane, generalized)
    int n_total, n_max, max_iteration;
    float thr2;
    double rel_fitness, rel_rmse;
    const double* tgt_rec;// [m_total, 8] colored: the targets' records (n [3], g [3], I, 0) ...
    const double* src_int;// [n_total] ... the sources' intensities ...
    double sg, sp;        // ... and sqrt(lambda_geometric), sqrt(1 - lambda_geometric)
    const double* src_cov;// [n_total, 6] generalized: the covariances of the unmoved sources ...
    const double* tgt_cov;// [m_total, 6] ... and of the targets
    int kernel;           // the robust evaluation (point-to-plane, colored): the kind of robust_kernel.h ...
    double kernel_k;      // ... and its scale
};

__device__ inline long first_slot(const IcpArgs& a, int p) { return (long)(a.src_off[p] / kIcpThreads) + p; }

__global__ void __launch_bounds__(256) k_icp_init(IcpArgs a, int B) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= B) return;
    IcpPair* st = a.state + p;
    for (int e = 0; e < 16; ++e) st->T[e] = a.init ? a.init[16 * (long)p + e] : (e % 5 == 0 ? 1.0 : 0.0);
    st->fitness = 0.0;
    st->rmse = 0.0;
    st->done = 0;
    st->pad = 0;
}

// Evaluate(T_it) of every live pair; grid (row blocks, pair).  ROBUST (EST 1 and 3): the terms under the call's kernel
template <int EST, bool ROBUST = false>
__global__ void __launch_bounds__(kIcpThreads) k_icp_evaluate(IcpArgs a, GridView g, int it) {
    constexpr int kTerms = icp_terms<EST>();
    __shared__ double s_sum[kIcpWaves][kTerms];
    __shared__ int s_cnt[kIcpWaves];
    const int p = blockIdx.y;
    const IcpPair* st = a.state + p;
    if (st->done) return;
    const int i0 = a.src_off[p], n = a.src_off[p + 1] - i0;
    if ((long)blockIdx.x * kIcpThreads >= n) return;
    const int j0 = a.tgt_off[p], m = a.tgt_off[p + 1] - j0;
    float T[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = (float)st->T[4 * r + c];
        T[9 + r] = (float)st->T[4 * r + 3];
    }
    const int i = blockIdx.x * kIcpThreads + threadIdx.x;
    float px = 0.f, py = 0.f, pz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
    float best = a.thr2;
    int bj = -1;
    if (i < n && m > 0) {
        const float* s = a.src + 3 * (long)(i0 + i);
        const float x = s[0], y = s[1], z = s[2];
        px = ((T[0] * x + T[1] * y) + T[2] * z) + T[9];
        py = ((T[3] * x + T[4] * y) + T[5] * z) + T[10];
        pz = ((T[6] * x + T[7] * y) + T[8] * z) + T[11];
        int cx, cy, cz;
        if (cell_coords(px, py, pz, g.hdr->inv_cell, &cx, &cy, &cz)) {      // false for a NaN or far-away point: no match
            const Slot* tab = g.tab + 2 * (long)j0;
            const unsigned tsize = 2u * (unsigned)m;
            for (int c = 0; c < 27; ++c) {
                const u64 key = cell_key(cx + c % 3 - 1, cy + (c / 3) % 3 - 1, cz + c / 9 - 1);
                unsigned sl_i = __umulhi(mix32(key), tsize);
                int cnt_c = 0, start = 0;
                for (unsigned probe = 0; probe < tsize; ++probe) {
                    const Slot sl = load_slot(&tab[sl_i]);
                    if (sl.key == key) { cnt_c = sl.cnt; start = sl.start; break; }
                    if (sl.key == kEmptyKey) break;
                    sl_i = sl_i + 1 == tsize ? 0 : sl_i + 1;
                }
                for (int e = 0; e < cnt_c; ++e) {
                    const float4 q = g.spts[start + e];
                    const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const int j = __float_as_int(q.w);
                    // (d2, index): the order of the points inside a cell is not defined, the lowest index of a tie is
                    if (d2 < best || (d2 == best && j < bj)) { best = d2; bj = j; qx = q.x; qy = q.y; qz = q.z; }
                }
            }
        }
    }
    const bool hit = bj >= 0;                 // best < thr2: bj is only ever set by a d2 below the start value or equal to a set one
    if (a.tr_corr && i < n) a.tr_corr[(long)it * a.n_total + i0 + i] = hit ? bj - j0 : -1;
    double v[kTerms];
    const double P[3] = {(double)px, (double)py, (double)pz}, Q[3] = {(double)qx, (double)qy, (double)qz};
    v[0] = hit ? (double)best : 0.0;
    if constexpr (EST == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            v[1 + r] = hit ? P[r] : 0.0;
            v[4 + r] = hit ? Q[r] : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[7 + 3 * r + c] = hit ? P[r] * Q[c] : 0.0;
        }
    } else if constexpr (EST == 2) {
        // W = (C_t[j] + R C_s[i] R^T)^-1 with R of T_k in float64; the terms of J0^T W J0 and -J0^T W d (gicp_terms.h)
        if (hit) {
            double R[9], Cs[6], Ct[6];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) R[3 * r + c] = st->T[4 * r + c];
            const double* cs = a.src_cov + 6 * (long)(i0 + i);
            const double* ct = a.tgt_cov + 6 * (long)bj;
#pragma unroll
            for (int e = 0; e < 6; ++e) { Cs[e] = cs[e]; Ct[e] = ct[e]; }
            gicp_terms(P, Q, R, Cs, Ct, v + 1);
        } else {
#pragma unroll
            for (int e = 1; e < kTerms; ++e) v[e] = 0.0;
        }
    } else if constexpr (EST == 3) {
        // the target's record in one aligned 64-byte read; the terms of JG JG^T + JI JI^T and -(JG rg + JI ri) (colored_terms.h)
        if (hit) {
            double rec[8];
            const double* tr = a.tgt_rec + 8 * (long)bj;
#pragma unroll
            for (int e = 0; e < 8; ++e) rec[e] = tr[e];
            if constexpr (ROBUST) colored_terms_robust(P, Q, rec, a.src_int[i0 + i], a.sg, a.sp, a.kernel, a.kernel_k, v + 1);
            else colored_terms(P, Q, rec, a.src_int[i0 + i], a.sg, a.sp, v + 1);
        } else {
#pragma unroll
            for (int e = 1; e < kTerms; ++e) v[e] = 0.0;
        }
    } else if constexpr (ROBUST) {
        // point-to-plane under the kernel: the terms below, each times the weight of the residual (robust_kernel.h)
        if (hit) {
            const double* nr = a.tgt_nrm + 3 * (long)bj;
            const double N[3] = {nr[0], nr[1], nr[2]};
            plane_terms_robust(P, Q, N, a.kernel, a.kernel_k, v + 1);
        } else {
#pragma unroll
            for (int e = 1; e < kTerms; ++e) v[e] = 0.0;
        }
    } else {
        // residual r = (p - q) . n and its Jacobian J = [p x n, n] about the moved point; both even in n as J J^T and J r
        double N[3] = {0.0, 0.0, 0.0};
        if (hit) { const double* nr = a.tgt_nrm + 3 * (long)bj; N[0] = nr[0]; N[1] = nr[1]; N[2] = nr[2]; }
        const double res = ((P[0] - Q[0]) * N[0] + (P[1] - Q[1]) * N[1]) + (P[2] - Q[2]) * N[2];
        const double J[6] = {P[1] * N[2] - P[2] * N[1], P[2] * N[0] - P[0] * N[2], P[0] * N[1] - P[1] * N[0], N[0], N[1], N[2]};
        int e = 1;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) v[e++] = hit ? J[r] * J[c] : 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) v[22 + r] = hit ? -(J[r] * res) : 0.0;
    }
    // fixed order: the wavefront's tree, then (below) the eight wavefronts one after the other
#pragma unroll
    for (int e = 0; e < kTerms; ++e)
#pragma unroll
        for (int sh = kWave / 2; sh >= 1; sh >>= 1) v[e] = v[e] + __shfl_down(v[e], sh, kWave);
    const int cnt = (int)__popcll(__ballot(hit));
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < kTerms; ++e) s_sum[wave][e] = v[e];
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    const long slot = first_slot(a, p) + blockIdx.x;
    if (threadIdx.x < kTerms) {
        double s = s_sum[0][threadIdx.x];
        for (int w = 1; w < kIcpWaves; ++w) s = s + s_sum[w][threadIdx.x];
        a.p_sum[kTerms * slot + threadIdx.x] = s;
    } else if (threadIdx.x == kTerms) {
        int c = 0;
        for (int w = 0; w < kIcpWaves; ++w) c += s_cnt[w];
        a.p_cnt[slot] = c;
    }
}

// the pair's outputs and its `done` word: every later launch leaves this pair alone
__device__ inline void icp_finish(const IcpArgs& a, int p, IcpPair* st, const double* T, double fitness, double rmse, double count,
                                  double iterations) {
    for (int e = 0; e < 16; ++e) a.out_t[16 * (long)p + e] = T[e];
    double* s = a.out_stats + 4 * (long)p;
    s[0] = fitness; s[1] = rmse; s[2] = count; s[3] = iterations;
    st->done = 1;
}

// After Evaluate(T_it): one wavefront per pair
template <int EST>
__global__ void __launch_bounds__(kWave) k_icp_update(IcpArgs a, int it) {
    constexpr int kTerms = icp_terms<EST>();
    __shared__ double s_tot[kTerms];
    __shared__ int s_count;
    const int p = blockIdx.x;
    IcpPair* st = a.state + p;
    if (st->done) return;
    const int n = a.src_off[p + 1] - a.src_off[p];
    const int nblk = n <= a.n_max ? (n + kIcpThreads - 1) / kIcpThreads : 0;
    const long slot0 = first_slot(a, p);
    if (threadIdx.x < kTerms) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s = s + a.p_sum[kTerms * (slot0 + b) + threadIdx.x];
        s_tot[threadIdx.x] = s;
    } else if (threadIdx.x == kTerms) {
        int c = 0;
        for (int b = 0; b < nblk; ++b) c += a.p_cnt[slot0 + b];
        s_count = c;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double T[16];
    for (int e = 0; e < 16; ++e) T[e] = st->T[e];
    if (it == 0) {
        bool finite = n <= a.n_max;           // a pair longer than the launch grid covers: no result rather than a partial one
        for (int e = 0; e < 16; ++e) finite = finite && fabs(T[e]) <= 1.79769313486231570815e308;
        if (!finite) {
            const double nan = __builtin_nan("");
            for (int e = 0; e < 16; ++e) T[e] = nan;
            icp_finish(a, p, st, T, nan, nan, nan, nan);
            return;
        }
    }
    const int count = s_count;
    const double sum = s_tot[0];
    const double fitness = n > 0 ? (double)count / (double)n : 0.0;
    const double rmse = count > 0 ? sqrt(sum / (double)count) : 0.0;
    const long tslot = (long)p * (a.max_iteration + 1) + it;
    if (a.tr_t)
        for (int e = 0; e < 16; ++e) a.tr_t[16 * tslot + e] = T[e];
    if (a.tr_counts) a.tr_counts[tslot] = count;
    if (a.tr_sums) a.tr_sums[tslot] = sum;
    const bool converged = it > 0 && fabs(fitness - st->fitness) < a.rel_fitness && fabs(rmse - st->rmse) < a.rel_rmse;
    st->fitness = fitness;
    st->rmse = rmse;
    if constexpr (EST != 0) {
        if (a.tr_sums27)
            for (int e = 0; e < 27; ++e) a.tr_sums27[27 * tslot + e] = s_tot[1 + e];
    }
    if (converged || it >= a.max_iteration || count < (EST == 1 ? 6 : 3)) {
        icp_finish(a, p, st, T, fitness, rmse, count, it);
        return;
    }
    if constexpr (EST != 0) {
        // Gauss-Newton step of sum r^2 (EST 2: of sum d^T W d; EST 3: of sum rg^2 + ri^2): (sum J J^T) x = -sum J r;
        // delta = Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)
        double x[6];
        // (EST 3: a source's or a target's intensity touches the right side alone, which the solve's pivots never see)
        bool rhs_finite = true;
        if constexpr (EST == 3)
            for (int e = 22; e < 28; ++e) rhs_finite = rhs_finite && fabs(s_tot[e]) <= 1.79769313486231570815e308;
        if (!rhs_finite || !solve_ldlt6(s_tot + 1, s_tot + 22, x)) {
            icp_finish(a, p, st, T, fitness, rmse, count, it);
            return;
        }
        const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
        const double R[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                             sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                             -sb,     cb * sa,                cb * ca};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                const double v = (R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c]) + R[3 * r + 2] * T[8 + c];
                st->T[4 * r + c] = c == 3 ? v + x[3 + r] : v;
            }
        return;
    }
    // Kabsch from the raw sums: centroids cs = sum p / count, ct = sum q / count, H = sum p q^T - (sum p) ct^T.  A difference
    // that is within 1e-12 of the two magnitudes it was taken from is their rounding residue and counts as 0: every row
    // matched to ONE target leaves H = 0 (degenerate by sigma_1 = 0), not a noise matrix with singular values of its own.
    double cs[3], ct[3], H[3][3], R[9], t[3];
    for (int r = 0; r < 3; ++r) { cs[r] = s_tot[1 + r] / (double)count; ct[r] = s_tot[4 + r] / (double)count; }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double spq = s_tot[7 + 3 * r + c], sc = s_tot[1 + r] * ct[c];
            const double h = spq - sc;
            H[r][c] = fabs(h) <= 1e-12 * (fabs(spq) + fabs(sc)) ? 0.0 : h;
        }
    if (!kabsch_from_covariance(H, cs, ct, R, t)) {
        icp_finish(a, p, st, T, fitness, rmse, count, it);
        return;
    }
    // T <- delta T (the bottom row stays)
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const double v = (R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c]) + R[3 * r + 2] * T[8 + c];
            st->T[4 * r + c] = c == 3 ? v + t[r] : v;
        }
}

// C = I - s n n^T of every normal (gicp_terms.h); one thread per row
constexpr int kCovThreads = 256;
constexpr int kCovMaxBlocks = 0x7FFFFFFF;

__global__ void __launch_bounds__(kCovThreads) k_cov_from_normals(const double* normals, long n, double s, double* cov) {
    const long i = (long)blockIdx.x * kCovThreads + threadIdx.x;
    if (i >= n) return;
    const double nr[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    double c[6];
    gicp_cov_of_normal(nr, s, c);
#pragma unroll
    for (int e = 0; e < 6; ++e) cov[6 * i + e] = c[e];
}

struct IcpWs {
    IcpPair* state;
    int* p_cnt;
    double* p_sum;
};

size_t icp_slots(int B, int n_total) { return (size_t)n_total / kIcpThreads + (size_t)B + 1; }

IcpWs carve_icp(Carver& cv, int B, int n_total, int terms) {
    IcpWs w;
    w.state = cv.take<IcpPair>((size_t)B);
    w.p_cnt = cv.take<int>(icp_slots(B, n_total));
    w.p_sum = cv.take<double>(icp_slots(B, n_total) * terms);
    return w;
}

// the launches of any estimator: init, then max_iteration + 1 evaluate / update pairs
template <int EST, bool ROBUST = false>
int icp_enqueue(const IcpArgs& a, const GridView& g, int B, hipStream_t st) {
    hipLaunchKernelGGL(k_icp_init, dim3((B + 255) / 256), dim3(256), 0, st, a, B);
    PCRCG_CHECK_LAUNCH();
    const dim3 eval_grid(a.n_max > 0 ? (a.n_max + kIcpThreads - 1) / kIcpThreads : 1, B);
    for (int it = 0; it <= a.max_iteration; ++it) {
        hipLaunchKernelGGL((k_icp_evaluate<EST, ROBUST>), eval_grid, dim3(kIcpThreads), 0, st, a, g, it);
        hipLaunchKernelGGL(k_icp_update<EST>, dim3(B), dim3(kWave), 0, st, a, it);
    }
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

// One call of any entry.  First what every entry takes, in the order of the ABI's argument lists (an entry initialises
// these from its own arguments, in that order); then its estimator and that estimator's own inputs, set by name.
struct IcpCall {
    const float* src;
    const int* src_off;
    int n_total, n_max;
    const int* tgt_off;
    int m_total;
    const void* grid;
    const double* init;
    int B;
    double max_correspondence_distance;
    int max_iteration;
    double relative_fitness, relative_rmse;
    double *out_transform, *out_stats;
    const pcrcg_icp_trace_ex* trace;                                // or null
    void* ws;
    size_t ws_bytes;
    void* stream;
    int estimation = kEstPoint;                                     // EST of the kernels
    const double* tgt_normals = nullptr;                            // point-to-plane
    const double *src_cov = nullptr, *tgt_cov = nullptr;            // generalized
    const double *tgt_rec = nullptr, *src_intensity = nullptr;      // colored
    double lambda_geometric = 0.0;
    bool robust = false;                                            // the robust entries: point-to-plane or colored under ...
    int kernel = kRobustL2;                                         // ... a kind of robust_kernel.h ...
    double kernel_k = 0.0;                                          // ... and its scale (kinds 2..5)
};

// Every entry's *_ws_bytes: 0 for sizes out of range
size_t icp_ws_bytes(int B, int n_total, int m_total, int max_iteration, int terms) {
    if (B < 1 || B > kIcpMaxBatch || n_total < 0 || m_total < 0 || max_iteration < 1 || max_iteration > kIcpMaxIteration) return 0;
    Carver cv(nullptr, 0);
    carve_icp(cv, B, n_total, terms);
    return cv.off;
}

#define ICP_CHECK_ARG(cond)                                          \
    do {                                                             \
        if (!(cond)) {                                               \
            set_error("%s: bad argument: %s", who, #cond);           \
            return PCRCG_EBADARG;                                    \
        }                                                            \
    } while (0)

// Every entry: the argument rules (reported under the entry's own name `who`), the workspace, the kernels' arguments, the launches
int icp_run(const char* who, const IcpCall& c) {
    ICP_CHECK_ARG(c.src_off && c.tgt_off && c.grid && c.out_transform && c.out_stats && c.ws);
    ICP_CHECK_ARG(c.B >= 1 && c.B <= kIcpMaxBatch);
    ICP_CHECK_ARG(c.n_total >= 0 && c.m_total >= 0 && c.n_max >= 0 && c.n_max <= c.n_total);
    ICP_CHECK_ARG(c.n_total == 0 || c.src);
    ICP_CHECK_ARG(c.max_correspondence_distance > 0.0 && c.max_correspondence_distance < 1e18);
    ICP_CHECK_ARG(c.max_iteration >= 1 && c.max_iteration <= kIcpMaxIteration);
    ICP_CHECK_ARG(c.relative_fitness >= 0.0 && c.relative_rmse >= 0.0);      // (false for a NaN)
    if (c.estimation == kEstPlane) ICP_CHECK_ARG(c.m_total == 0 || c.tgt_normals);
    if (c.estimation == kEstGeneralized) {
        ICP_CHECK_ARG(c.n_total == 0 || c.src_cov);
        ICP_CHECK_ARG(c.m_total == 0 || c.tgt_cov);
    }
    if (c.estimation == kEstColored) {
        ICP_CHECK_ARG(c.lambda_geometric >= 0.0 && c.lambda_geometric <= 1.0);   // (false for a NaN)
        ICP_CHECK_ARG(c.n_total == 0 || c.src_intensity);
        ICP_CHECK_ARG(c.m_total == 0 || c.tgt_rec);
    }
    ICP_CHECK_ARG(c.kernel >= 0 && c.kernel < kRobustKinds);
    ICP_CHECK_ARG(c.kernel < kRobustHuber || (c.kernel_k > 0.0 && c.kernel_k <= 1.79769313486231570815e308));  // (false for a NaN)
    const bool point = c.estimation == kEstPoint;
    Carver cv(c.ws, c.ws_bytes);
    IcpWs w = carve_icp(cv, c.B, c.n_total, point ? kIcpTerms : kIcpPlaneTerms);
    if (!cv.ok()) {
        set_error("%s: workspace too small (%zu needed, %zu given)", who, cv.off, cv.cap);
        return PCRCG_EWORKSPACE;
    }
    bool ok;
    GridView g = grid_view(const_cast<void*>(c.grid), grid_bytes(c.m_total, c.B), c.m_total, c.B, &ok);
    const bool colored = c.estimation == kEstColored;
    const pcrcg_icp_trace_ex none = {nullptr, nullptr, nullptr, nullptr, nullptr}, &tr = c.trace ? *c.trace : none;
    IcpArgs a;
    a.src = c.src; a.src_off = c.src_off; a.tgt_off = c.tgt_off; a.init = c.init;
    a.state = w.state; a.p_cnt = w.p_cnt; a.p_sum = w.p_sum;
    a.out_t = c.out_transform; a.out_stats = c.out_stats;
    a.tr_t = tr.transforms; a.tr_counts = tr.counts; a.tr_sums = tr.sums; a.tr_corr = tr.corr;
    a.tgt_nrm = c.tgt_normals;
    a.tr_sums27 = point ? nullptr : tr.sums27;
    a.n_total = c.n_total; a.n_max = c.n_max; a.max_iteration = c.max_iteration;
    a.thr2 = (float)(c.max_correspondence_distance * c.max_correspondence_distance);
    a.rel_fitness = c.relative_fitness; a.rel_rmse = c.relative_rmse;
    a.tgt_rec = c.tgt_rec; a.src_int = c.src_intensity;
    a.sg = colored ? sqrt(c.lambda_geometric) : 0.0;
    a.sp = colored ? sqrt(1.0 - c.lambda_geometric) : 0.0;
    a.src_cov = c.src_cov; a.tgt_cov = c.tgt_cov;
    a.kernel = c.kernel; a.kernel_k = c.kernel_k;
    const hipStream_t st = as_stream(c.stream);
    if (c.robust)               // (after the plain estimators' kernels in the code object)
        return c.estimation == kEstColored ? icp_enqueue<kEstColored, true>(a, g, c.B, st) : icp_enqueue<kEstPlane, true>(a, g, c.B, st);
    switch (c.estimation) {     // (the cases' order is the kernels' order in the code object: append)
    case kEstGeneralized: return icp_enqueue<kEstGeneralized>(a, g, c.B, st);
    case kEstColored: return icp_enqueue<kEstColored>(a, g, c.B, st);
    case kEstPoint: return icp_enqueue<kEstPoint>(a, g, c.B, st);
    default: return icp_enqueue<kEstPlane>(a, g, c.B, st);
    }
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_icp_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration) {
    return icp_ws_bytes(B, n_total, m_total, max_iteration, kIcpTerms);
}

int pcrcg_icp_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                    const void* grid, const double* init, int B, double max_correspondence_distance, int max_iteration,
                    double relative_fitness, double relative_rmse, double* out_transform, double* out_stats,
                    const pcrcg_icp_trace* trace, void* ws, size_t ws_bytes, void* stream) {
    pcrcg_icp_trace_ex tr = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (trace) { tr.transforms = trace->transforms; tr.counts = trace->counts; tr.sums = trace->sums; tr.corr = trace->corr; }
    IcpCall c = {src, src_off, n_total, n_max, tgt_off, m_total, grid, init, B, max_correspondence_distance, max_iteration,
                 relative_fitness, relative_rmse, out_transform, out_stats, &tr, ws, ws_bytes, stream};
    return icp_run(__func__, c);
}

size_t pcrcg_icp_batch_ex_ws_bytes(int B, int n_total, int m_total, int max_iteration) {
    return icp_ws_bytes(B, n_total, m_total, max_iteration, kIcpPlaneTerms);
}

int pcrcg_icp_batch_ex(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                       const void* grid, const double* init, int B, double max_correspondence_distance, int max_iteration,
                       double relative_fitness, double relative_rmse, int estimation, const double* tgt_normals,
                       double* out_transform, double* out_stats, const pcrcg_icp_trace_ex* trace, void* ws, size_t ws_bytes,
                       void* stream) {
    const char* who = __func__;
    ICP_CHECK_ARG(estimation == 0 || estimation == 1);       // this entry's two: point-to-point and point-to-plane
    IcpCall c = {src, src_off, n_total, n_max, tgt_off, m_total, grid, init, B, max_correspondence_distance, max_iteration,
                 relative_fitness, relative_rmse, out_transform, out_stats, trace, ws, ws_bytes, stream};
    c.estimation = estimation;
    c.tgt_normals = tgt_normals;
    return icp_run(who, c);
}

int pcrcg_covariances_from_normals(const double* normals, long n, double epsilon, double* cov, void* stream) {
    PCRCG_CHECK_ARG(epsilon > 0.0 && epsilon <= 1.0);      // (false for a NaN)
    PCRCG_CHECK_ARG(n >= 0 && n <= (long)kCovMaxBlocks * kCovThreads);
    PCRCG_CHECK_ARG(n == 0 || (normals && cov));
    if (n == 0) return PCRCG_OK;
    hipLaunchKernelGGL(k_cov_from_normals, dim3((unsigned)((n + kCovThreads - 1) / kCovThreads)), dim3(kCovThreads), 0,
                       as_stream(stream), normals, n, 1.0 - epsilon, cov);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

size_t pcrcg_gicp_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration) {
    return icp_ws_bytes(B, n_total, m_total, max_iteration, kIcpPlaneTerms);
}

int pcrcg_gicp_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                     const void* grid, const double* init, int B, double max_correspondence_distance, int max_iteration,
                     double relative_fitness, double relative_rmse, const double* src_cov, const double* tgt_cov,
                     double* out_transform, double* out_stats, const pcrcg_icp_trace_ex* trace, void* ws, size_t ws_bytes,
                     void* stream) {
    IcpCall c = {src, src_off, n_total, n_max, tgt_off, m_total, grid, init, B, max_correspondence_distance, max_iteration,
                 relative_fitness, relative_rmse, out_transform, out_stats, trace, ws, ws_bytes, stream};
    c.estimation = kEstGeneralized;
    c.src_cov = src_cov;
    c.tgt_cov = tgt_cov;
    return icp_run(__func__, c);
}

size_t pcrcg_colored_icp_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration) {
    return icp_ws_bytes(B, n_total, m_total, max_iteration, kIcpPlaneTerms);
}

int pcrcg_colored_icp_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                            const void* grid, const double* init, int B, double max_correspondence_distance, int max_iteration,
                            double relative_fitness, double relative_rmse, double lambda_geometric, const double* tgt_rec,
                            const double* src_intensity, double* out_transform, double* out_stats,
                            const pcrcg_icp_trace_ex* trace, void* ws, size_t ws_bytes, void* stream) {
    IcpCall c = {src, src_off, n_total, n_max, tgt_off, m_total, grid, init, B, max_correspondence_distance, max_iteration,
                 relative_fitness, relative_rmse, out_transform, out_stats, trace, ws, ws_bytes, stream};
    c.estimation = kEstColored;
    c.lambda_geometric = lambda_geometric;
    c.tgt_rec = tgt_rec;
    c.src_intensity = src_intensity;
    return icp_run(__func__, c);
}

size_t pcrcg_icp_plane_robust_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration) {
    return icp_ws_bytes(B, n_total, m_total, max_iteration, kIcpPlaneTerms);
}

int pcrcg_icp_plane_robust_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                                 const void* grid, const double* init, int B, double max_correspondence_distance,
                                 int max_iteration, double relative_fitness, double relative_rmse, const double* tgt_normals,
                                 int kernel, double kernel_k, double* out_transform, double* out_stats,
                                 const pcrcg_icp_trace_ex* trace, void* ws, size_t ws_bytes, void* stream) {
    IcpCall c = {src, src_off, n_total, n_max, tgt_off, m_total, grid, init, B, max_correspondence_distance, max_iteration,
                 relative_fitness, relative_rmse, out_transform, out_stats, trace, ws, ws_bytes, stream};
    c.estimation = kEstPlane;
    c.tgt_normals = tgt_normals;
    c.robust = true;
    c.kernel = kernel;
    c.kernel_k = kernel_k;
    return icp_run(__func__, c);
}

size_t pcrcg_colored_icp_robust_batch_ws_bytes(int B, int n_total, int m_total, int max_iteration) {
    return icp_ws_bytes(B, n_total, m_total, max_iteration, kIcpPlaneTerms);
}

int pcrcg_colored_icp_robust_batch(const float* src, const int* src_off, int n_total, int n_max, const int* tgt_off, int m_total,
                                   const void* grid, const double* init, int B, double max_correspondence_distance,
                                   int max_iteration, double relative_fitness, double relative_rmse, double lambda_geometric,
                                   const double* tgt_rec, const double* src_intensity, int kernel, double kernel_k,
                                   double* out_transform, double* out_stats, const pcrcg_icp_trace_ex* trace, void* ws,
                                   size_t ws_bytes, void* stream) {
    IcpCall c = {src, src_off, n_total, n_max, tgt_off, m_total, grid, init, B, max_correspondence_distance, max_iteration,
                 relative_fitness, relative_rmse, out_transform, out_stats, trace, ws, ws_bytes, stream};
    c.estimation = kEstColored;
    c.lambda_geometric = lambda_geometric;
    c.tgt_rec = tgt_rec;
    c.src_intensity = src_intensity;
    c.robust = true;
    c.kernel = kernel;
    c.kernel_k = kernel_k;
    return icp_run(__func__, c);
}

#undef ICP_CHECK_ARG

}  // extern "C"
