// gicp_terms.h -- the per-correspondence arithmetic of Generalized ICP (icp.hip, EST = 2; include/pcrcg.h "Generalized ICP"):
// the 3 x 3 metric of one correspondence and its 27 terms of the 6 x 6 Gauss-Newton system, and the covariance of a normal.
// Plain C++ with no HIP types (host and device): icp.hip is compiled with -ffp-contract=off, and tests/host/gicp_terms_driver.cpp
// compiles this text for the host, so every operation below rounds where it is written.
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

// C = I - (1 - epsilon) n n^T as (xx, xy, xz, yy, yz, zz); s = 1 - epsilon.  Every entry is delta - (s n_r) n_c: even in n.
PCRCG_HD inline void gicp_cov_of_normal(const double* n, double s, double* cov) {
    const double a0 = s * n[0], a1 = s * n[1], a2 = s * n[2];
    cov[0] = 1.0 - a0 * n[0];
    cov[1] = 0.0 - a0 * n[1];
    cov[2] = 0.0 - a0 * n[2];
    cov[3] = 1.0 - a1 * n[1];
    cov[4] = 0.0 - a1 * n[2];
    cov[5] = 1.0 - a2 * n[2];
}

// W = (Ct + R Cs R^T)^-1 as (xx, xy, xz, yy, yz, zz).  R [9] row-major; Cs, Ct packed like W.
//   X = R Cs, the full 3 x 3, X[r][c] = ((R[r][0] S[0][c] + R[r][1] S[1][c]) + R[r][2] S[2][c]);
//   M[r][c] = Ct[r][c] + ((X[r][0] R[c][0] + X[r][1] R[c][1]) + X[r][2] R[c][2]) for r <= c;
//   the six cofactors, det = ((m00 c00 + m01 c01) + m02 c02), W = cofactor / det (six divisions).
// Nothing is tested: a metric that is not finite, or singular, gives entries that are not finite.
PCRCG_HD inline void gicp_metric(const double* R, const double* Cs, const double* Ct, double* W) {
    const double S[3][3] = {{Cs[0], Cs[1], Cs[2]}, {Cs[1], Cs[3], Cs[4]}, {Cs[2], Cs[4], Cs[5]}};
    double X[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) X[r][c] = (R[3 * r] * S[0][c] + R[3 * r + 1] * S[1][c]) + R[3 * r + 2] * S[2][c];
    double m[6];
    for (int r = 0, e = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c, ++e) m[e] = Ct[e] + ((X[r][0] * R[3 * c] + X[r][1] * R[3 * c + 1]) + X[r][2] * R[3 * c + 2]);
    const double m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[3], m12 = m[4], m22 = m[5];
    const double c00 = m11 * m22 - m12 * m12;
    const double c01 = m02 * m12 - m01 * m22;
    const double c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02;
    const double c12 = m01 * m02 - m00 * m12;
    const double c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    W[0] = c00 / det;
    W[1] = c01 / det;
    W[2] = c02 / det;
    W[3] = c11 / det;
    W[4] = c12 / det;
    W[5] = c22 / det;
}

// The 27 terms of one correspondence: the upper triangle of J0^T W J0 row by row (21), then -J0^T W d (6), with
// J0 = [-[p]x | I] and d = p - q.  With w_r the rows of W:
//   g_r = p x w_r (each component a b - c d): the rows of W (-[p]x);
//   the rotation block's row a, columns c >= a: the a-th component of p x (g_0[c], g_1[c], g_2[c]);
//   the mixed block [a][3 + c] = g_c[a]; the translation block = W;
//   e_r = ((w_r0 d0 + w_r1 d1) + w_r2 d2); the right side = -(p x e), -e.
PCRCG_HD inline void gicp_terms(const double* p, const double* q, const double* R, const double* Cs, const double* Ct,
                                double* out) {
    double W6[6];
    gicp_metric(R, Cs, Ct, W6);
    const double W[3][3] = {{W6[0], W6[1], W6[2]}, {W6[1], W6[3], W6[4]}, {W6[2], W6[4], W6[5]}};
    const double px = p[0], py = p[1], pz = p[2];
    double g[3][3];
    for (int r = 0; r < 3; ++r) {
        g[r][0] = py * W[r][2] - pz * W[r][1];
        g[r][1] = pz * W[r][0] - px * W[r][2];
        g[r][2] = px * W[r][1] - py * W[r][0];
    }
    out[0] = py * g[2][0] - pz * g[1][0];
    out[1] = py * g[2][1] - pz * g[1][1];
    out[2] = py * g[2][2] - pz * g[1][2];
    out[3] = g[0][0];
    out[4] = g[1][0];
    out[5] = g[2][0];
    out[6] = pz * g[0][1] - px * g[2][1];
    out[7] = pz * g[0][2] - px * g[2][2];
    out[8] = g[0][1];
    out[9] = g[1][1];
    out[10] = g[2][1];
    out[11] = px * g[1][2] - py * g[0][2];
    out[12] = g[0][2];
    out[13] = g[1][2];
    out[14] = g[2][2];
    out[15] = W6[0];
    out[16] = W6[1];
    out[17] = W6[2];
    out[18] = W6[3];
    out[19] = W6[4];
    out[20] = W6[5];
    const double d0 = px - q[0], d1 = py - q[1], d2 = pz - q[2];
    double e[3];
    for (int r = 0; r < 3; ++r) e[r] = (W[r][0] * d0 + W[r][1] * d1) + W[r][2] * d2;
    out[21] = -(py * e[2] - pz * e[1]);
    out[22] = -(pz * e[0] - px * e[2]);
    out[23] = -(px * e[1] - py * e[0]);
    out[24] = -e[0];
    out[25] = -e[1];
    out[26] = -e[2];
}

}  // namespace
}  // namespace pcrcg
