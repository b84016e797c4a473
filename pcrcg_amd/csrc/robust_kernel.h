// robust_kernel.h -- the robust loss kernels of the ICP family (icp.hip, the robust evaluation of EST = 1 and EST = 3;
// include/pcrcg.h "Robust kernels"): open3d's RobustKernel::Weight as one function of a kind, a scale k and a residual r,
// and the 27 weighted terms one point-to-plane correspondence adds to the 6 x 6 Gauss-Newton system (colored ICP's are
// colored_terms.h's colored_terms_robust).
// Plain C++ with no HIP types (host and device): icp.hip is compiled with -ffp-contract=off, and
// tests/host/robust_kernel_driver.cpp compiles this text for the host, so every operation below rounds where it is written.
// Basic IEEE operations only (+ - * / and comparisons; no pow, no library call): tests/robust_ref.py restates them in numpy
// bit for bit.
#pragma once

#ifndef PCRCG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCRCG_HD __host__ __device__
#else
#define PCRCG_HD
#endif
#endif

namespace pcrcg {
namespace {

constexpr int kRobustL2 = 0, kRobustL1 = 1, kRobustHuber = 2, kRobustCauchy = 3, kRobustGM = 4, kRobustTukey = 5;
constexpr int kRobustKinds = 6;
// open3d's L1 weight is 1 / |r|: infinite at r = 0, where it turns the whole system into NaN.  Here |r| is held at this floor
// -- the one departure from open3d: a correspondence that lies exactly on its target's plane is an ordinary one.
constexpr double kL1Floor = 1e-12;

// max and min that keep a NaN: with a NaN on either side both comparisons are false and the sum, a NaN, is returned.
PCRCG_HD inline double robust_max(double a, double b) { return a >= b ? a : (b > a ? b : a + b); }
PCRCG_HD inline double robust_min(double a, double b) { return a <= b ? a : (b < a ? b : a + b); }

// The weight of a residual r: the factor its row of the system is multiplied with.  k is the kind's scale (not read by L2
// and L1).  A NaN residual gives a NaN weight (L2: 1.0); an infinite one gives 0.
//   L2     1.0
//   L1     1.0 / max(|r|, kL1Floor)
//   Huber  k / max(|r|, k)
//   Cauchy 1.0 / (1.0 + (r / k) (r / k))
//   GM     k / ((k + r r) (k + r r))
//   Tukey  t = min(1.0, |r| / k); u = 1.0 - t t; u u
PCRCG_HD inline double robust_weight(int kind, double k, double r) {
    const double a = __builtin_fabs(r);
    switch (kind) {
    case kRobustL1: return 1.0 / robust_max(a, kL1Floor);
    case kRobustHuber: return k / robust_max(a, k);
    case kRobustCauchy: {
        const double t = r / k;
        return 1.0 / (1.0 + t * t);
    }
    case kRobustGM: {
        const double s = k + r * r;
        return k / (s * s);
    }
    case kRobustTukey: {
        const double t = robust_min(1.0, a / k);
        const double u = 1.0 - t * t;
        return u * u;
    }
    default: return 1.0;
    }
}

// The 27 terms of one point-to-plane correspondence under a kernel: p the moved source point, q its target, n the target's
// normal; res = (((p - q) . n)), J = [p x n | n], w = robust_weight(kind, k, res); the upper triangle of w (J J^T) row by
// row (21), then w (-(J res)) (6).  The weight multiplies the finished term of the plain estimator: kind 0 gives its bits.
PCRCG_HD inline void plane_terms_robust(const double* p, const double* q, const double* n, int kind, double k, double* out) {
    const double res = ((p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1]) + (p[2] - q[2]) * n[2];
    const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
    const double w = robust_weight(kind, k, res);
    int e = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) out[e++] = w * (J[r] * J[c]);
    for (int r = 0; r < 6; ++r) out[21 + r] = w * (-(J[r] * res));
}

}  // namespace
}  // namespace pcrcg
