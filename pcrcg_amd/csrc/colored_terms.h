// colored_terms.h -- the per-point and per-correspondence arithmetic of colored ICP (colored.hip; icp.hip, EST = 3;
// include/pcrcg.h "Colored ICP"): one row of a target point's colour-gradient fit, the fit's last row, and the 27 terms one
// correspondence adds to the 6 x 6 Gauss-Newton system of the joint colour / geometry objective, plain or under a robust kernel.
// Plain C++ with no HIP types (host and device): both kernels are compiled with -ffp-contract=off, and
// tests/host/colored_terms_driver.cpp compiles this text for the host, so every operation below rounds where it is written.
#pragma once

#include "robust_kernel.h"

#ifndef PCRCG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCRCG_HD __host__ __device__
#else
#define PCRCG_HD
#endif
#endif

namespace pcrcg {
namespace {

// One row of the gradient fit of the point vt with the normal nt: the neighbour a is projected onto the tangent plane,
//   dot = (((a - vt) . nt)), A_r = (a_r - dot nt_r) - vt_r, b = Ia - Ik,
// and the row's nine products are out = (A0 A0, A0 A1, A0 A2, A1 A1, A1 A2, A2 A2, A0 b, A1 b, A2 b).
PCRCG_HD inline void colored_gradient_row(const double* vt, const double* nt, const double* a, double Ia, double Ik, double* out) {
    const double d0 = a[0] - vt[0], d1 = a[1] - vt[1], d2 = a[2] - vt[2];
    const double dot = (d0 * nt[0] + d1 * nt[1]) + d2 * nt[2];
    const double A0 = (a[0] - dot * nt[0]) - vt[0];
    const double A1 = (a[1] - dot * nt[1]) - vt[1];
    const double A2 = (a[2] - dot * nt[2]) - vt[2];
    const double b = Ia - Ik;
    out[0] = A0 * A0;
    out[1] = A0 * A1;
    out[2] = A0 * A2;
    out[3] = A1 * A1;
    out[4] = A1 * A2;
    out[5] = A2 * A2;
    out[6] = A0 * b;
    out[7] = A1 * b;
    out[8] = A2 * b;
}

// The fit's last row (nn - 1) nt with the right side 0, which holds the gradient in the tangent plane: with w = nn - 1 and
// r = w nt, sums[e] = sums[e] + r_r r_c over the six entries of the upper triangle.  nn is the list's length.
PCRCG_HD inline void colored_gradient_last_row(const double* nt, int nn, double* sums) {
    const double w = (double)(nn - 1);
    const double r0 = w * nt[0], r1 = w * nt[1], r2 = w * nt[2];
    sums[0] = sums[0] + r0 * r0;
    sums[1] = sums[1] + r0 * r1;
    sums[2] = sums[2] + r0 * r2;
    sums[3] = sums[3] + r1 * r1;
    sums[4] = sums[4] + r1 * r2;
    sums[5] = sums[5] + r2 * r2;
}

// The 27 terms of one correspondence: the upper triangle of JG JG^T + JI JI^T row by row (21, the geometric product first),
// then -(JG rg + JI ri) (6).  p the moved source point, q its target, rec = (n [3], g [3], It, 0) the target's record, Is the
// source's intensity, sg = sqrt(lambda_geometric), sp = sqrt(1 - lambda_geometric).
//   rG = (((p - q) . n)); J = [p x n | n] (a cross product is a b - c d per component); JG = sg J, rg = sg rG;
//   pproj = p - rG n; I0 = (((g . (pproj - q))) + It); gn = ((g . n)); gM = -(g - gn n);
//   JI = sp [p x gM | gM]; ri = sp (Is - I0).
// Dot products are ((x + y) + z).  Nothing is tested: a value that is not finite gives terms that are not finite.
// ROBUST: each of the two rows carries the weight of its own scaled residual, wg = robust_weight(kind, k, rg) and
// wi = robust_weight(kind, k, ri) (robust_kernel.h), as open3d weights them: the terms are
// wg (JG_r JG_c) + wi (JI_r JI_c) and -(wg (JG_r rg) + wi (JI_r ri)), in the order of operations of the plain terms, so kind 0
// (both weights 1.0) gives their bits.
template <bool ROBUST>
PCRCG_HD inline void colored_terms_of(const double* p, const double* q, const double* rec, double Is, double sg, double sp,
                                      int kind, double k, double* out) {
    const double px = p[0], py = p[1], pz = p[2];
    const double n0 = rec[0], n1 = rec[1], n2 = rec[2];
    const double g0 = rec[3], g1 = rec[4], g2 = rec[5];
    const double rG = ((px - q[0]) * n0 + (py - q[1]) * n1) + (pz - q[2]) * n2;
    const double rg = sg * rG;
    const double e0 = (px - rG * n0) - q[0], e1 = (py - rG * n1) - q[1], e2 = (pz - rG * n2) - q[2];
    const double I0 = ((g0 * e0 + g1 * e1) + g2 * e2) + rec[6];
    const double ri = sp * (Is - I0);
    const double gn = (g0 * n0 + g1 * n1) + g2 * n2;
    const double m0 = -(g0 - gn * n0), m1 = -(g1 - gn * n1), m2 = -(g2 - gn * n2);
    const double JG[6] = {sg * (py * n2 - pz * n1), sg * (pz * n0 - px * n2), sg * (px * n1 - py * n0), sg * n0, sg * n1, sg * n2};
    const double JI[6] = {sp * (py * m2 - pz * m1), sp * (pz * m0 - px * m2), sp * (px * m1 - py * m0), sp * m0, sp * m1, sp * m2};
    int e = 0;
    if constexpr (ROBUST) {
        const double wg = robust_weight(kind, k, rg), wi = robust_weight(kind, k, ri);
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) out[e++] = wg * (JG[r] * JG[c]) + wi * (JI[r] * JI[c]);
        for (int r = 0; r < 6; ++r) out[21 + r] = -(wg * (JG[r] * rg) + wi * (JI[r] * ri));
    } else {
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) out[e++] = JG[r] * JG[c] + JI[r] * JI[c];
        for (int r = 0; r < 6; ++r) out[21 + r] = -(JG[r] * rg + JI[r] * ri);
    }
}

PCRCG_HD inline void colored_terms(const double* p, const double* q, const double* rec, double Is, double sg, double sp,
                                   double* out) {
    colored_terms_of<false>(p, q, rec, Is, sg, sp, 0, 0.0, out);
}

PCRCG_HD inline void colored_terms_robust(const double* p, const double* q, const double* rec, double Is, double sg, double sp,
                                          int kind, double k, double* out) {
    colored_terms_of<true>(p, q, rec, Is, sg, sp, kind, k, out);
}

}  // namespace
}  // namespace pcrcg
