// kabsch.h -- the float64 rigid fit from a 3 x 3 cross-covariance: the second half of the Kabsch fit, shared by RANSAC's
// hypotheses (register.hip) and the ICP update (icp.hip).  Both files are compiled with -ffp-contract=off.
#pragma once
#include "common.h"

namespace pcrcg {
namespace {

// H = sum (ps - cs)(pt - ct)^T (overwritten), cs / ct the centroids: H = U S V^T, R = V diag(1, 1, det(V U^T)) U^T (row-major),
// t = ct - R cs.  Returns false, with R and t untouched, when the sample is degenerate: sigma_2 <= 1e-12 sigma_1.
__device__ __forceinline__ bool kabsch_from_covariance(double H[3][3], const double* cs, const double* ct, double* R, double* t) {
    // one-sided Jacobi: rotate the columns of B = H V until they are orthogonal; then sigma_c = |B[:, c]|, u_c = B[:, c] / sigma_c
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 3; ++r) { al += H[r][p] * H[r][p]; be += H[r][q] * H[r][q]; ga += H[r][p] * H[r][q]; }
                if (ga == 0.0 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cc = 1.0 / sqrt(1.0 + tt * tt), sn = cc * tt;
                for (int r = 0; r < 3; ++r) {
                    const double hp = H[r][p], hq = H[r][q];
                    H[r][p] = cc * hp - sn * hq;
                    H[r][q] = sn * hp + cc * hq;
                    const double vp = V[r][p], vq = V[r][q];
                    V[r][p] = cc * vp - sn * vq;
                    V[r][q] = sn * vp + cc * vq;
                }
            }
        if (!rotated) break;
    }
    double sg[3];
    for (int c = 0; c < 3; ++c) sg[c] = sqrt((H[0][c] * H[0][c] + H[1][c] * H[1][c]) + H[2][c] * H[2][c]);
    int i1 = 0;
    for (int c = 1; c < 3; ++c) if (sg[c] > sg[i1]) i1 = c;
    int i2 = i1 == 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c) if (c != i1 && sg[c] > sg[i2]) i2 = c;
    if (!(sg[i2] > 1e-12 * sg[i1])) return false;                 // degenerate sample (also catches sigma_1 = 0)
    double u1[3], u2[3], v1[3], v2[3];
    for (int r = 0; r < 3; ++r) {
        u1[r] = H[r][i1] / sg[i1]; u2[r] = H[r][i2] / sg[i2];
        v1[r] = V[r][i1]; v2[r] = V[r][i2];
    }
    // R u1 = v1, R u2 = v2 and R proper: R (u1 x u2) = v1 x v2 -- the reflection fix without a third singular vector
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (v1[r] * u1[c] + v2[r] * u2[c]) + v3[r] * u3[c];
    for (int r = 0; r < 3; ++r) t[r] = ct[r] - ((R[3 * r] * cs[0] + R[3 * r + 1] * cs[1]) + R[3 * r + 2] * cs[2]);
    return true;
}

}  // namespace
}  // namespace pcrcg
