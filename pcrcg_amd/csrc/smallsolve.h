// smallsolve.h -- three float64 dense solvers that run in ONE lane: the eigenvector of a symmetric 3 x 3 matrix's smallest
// eigenvalue (normals.hip), the diagonally pivoted LDL^T solve of a symmetric 6 x 6 system (icp.hip, point-to-plane) and the
// same solve of a 3 x 3 system (colored.hip).
// Plain C++ (host and device): both files are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace pcrcg {
namespace {

// C = (xx, xy, xz, yy, yz, zz).  Cyclic Jacobi on the symmetric matrix; n = the column of the accumulated rotations that
// belongs to the smallest diagonal entry (the lowest index among equal ones), normalised.  Returns false, n untouched, when
// C is identically zero or holds a value that is not finite.
__host__ __device__ inline bool smallest_eigenvector_sym3(const double* C, double* n) {
    double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    bool zero = true, finite = true;
    for (int e = 0; e < 6; ++e) {
        zero = zero && C[e] == 0.0;
        finite = finite && fabs(C[e]) <= 1.79769313486231570815e308;
    }
    if (zero || !finite) return false;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                // (an off-diagonal entry that small no longer moves either diagonal entry)
                if (apq == 0.0 || fabs(apq) <= 1e-17 * sqrt(fabs(A[p][p] * A[q][q]))) continue;
                rotated = true;
                const double zeta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cc = 1.0 / sqrt(1.0 + tt * tt), sn = cc * tt;
                // A <- J^T A J with J = [[cc, sn], [-sn, cc]] on rows / columns p, q
                for (int r = 0; r < 3; ++r) {
                    const double ap = A[r][p], aq = A[r][q];
                    A[r][p] = cc * ap - sn * aq;
                    A[r][q] = sn * ap + cc * aq;
                }
                for (int c = 0; c < 3; ++c) {
                    const double ap = A[p][c], aq = A[q][c];
                    A[p][c] = cc * ap - sn * aq;
                    A[q][c] = sn * ap + cc * aq;
                }
                A[p][q] = 0.0;
                A[q][p] = 0.0;
                for (int r = 0; r < 3; ++r) {
                    const double vp = V[r][p], vq = V[r][q];
                    V[r][p] = cc * vp - sn * vq;
                    V[r][q] = sn * vp + cc * vq;
                }
            }
        if (!rotated) break;
    }
    int k = 0;
    for (int c = 1; c < 3; ++c)
        if (A[c][c] < A[k][k]) k = c;
    const double len = sqrt((V[0][k] * V[0][k] + V[1][k] * V[1][k]) + V[2][k] * V[2][k]);
    if (!(len > 0.0)) return false;
    for (int r = 0; r < 3; ++r) n[r] = V[r][k] / len;
    return true;
}

// A x = b for a symmetric 6 x 6 A given by its upper triangle, row by row (21 values: 00 01 .. 05 11 12 .. 55), by LDL^T with
// diagonal pivoting: step k takes the largest remaining diagonal entry (the lowest index among equal ones) as the pivot d_k.
// Returns false, x untouched, as soon as a pivot is not above 1e-12 times the largest pivot so far (for a positive
// semi-definite A the pivots do not grow, so that is "smallest pivot <= 1e-12 largest"; a NaN fails the comparison too).
__host__ __device__ inline bool solve_ldlt6(const double* upper, const double* b, double* x) {
    double A[6][6], y[6];
    int perm[6];
    for (int r = 0, e = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c, ++e) { A[r][c] = upper[e]; A[c][r] = upper[e]; }
    for (int r = 0; r < 6; ++r) { perm[r] = r; y[r] = b[r]; }
    double dmax = 0.0;
    for (int k = 0; k < 6; ++k) {
        int piv = k;
        for (int r = k + 1; r < 6; ++r)
            if (A[r][r] > A[piv][piv]) piv = r;
        if (piv != k) {
            for (int c = 0; c < 6; ++c) { const double t = A[k][c]; A[k][c] = A[piv][c]; A[piv][c] = t; }
            for (int r = 0; r < 6; ++r) { const double t = A[r][k]; A[r][k] = A[r][piv]; A[r][piv] = t; }
            { const double t = y[k]; y[k] = y[piv]; y[piv] = t; }
            { const int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t; }
        }
        const double d = A[k][k];
        if (d > dmax) dmax = d;
        if (!(d > 1e-12 * dmax) || !(d > 0.0)) return false;
        // column k of L below the diagonal, then the Schur complement of the trailing block (kept symmetric)
        for (int r = k + 1; r < 6; ++r) A[r][k] = A[r][k] / d;
        for (int r = k + 1; r < 6; ++r)
            for (int c = k + 1; c <= r; ++c) {
                const double v = A[r][c] - A[r][k] * (d * A[c][k]);
                A[r][c] = v;
                A[c][r] = v;
            }
    }
    // L z = y, D w = z, L^T u = w; x[perm] = u
    for (int r = 1; r < 6; ++r)
        for (int c = 0; c < r; ++c) y[r] = y[r] - A[r][c] * y[c];
    for (int r = 0; r < 6; ++r) y[r] = y[r] / A[r][r];
    for (int r = 4; r >= 0; --r)
        for (int c = r + 1; c < 6; ++c) y[r] = y[r] - A[c][r] * y[c];
    for (int r = 0; r < 6; ++r) x[perm[r]] = y[r];
    return true;
}

// rows / columns i and j of the symmetric 3 x 3 system exchanged (i, j constants where solve_ldlt3 calls this)
__host__ __device__ inline void ldlt3_swap(double (&A)[3][3], double (&y)[3], int (&perm)[3], int i, int j) {
    for (int c = 0; c < 3; ++c) { const double t = A[i][c]; A[i][c] = A[j][c]; A[j][c] = t; }
    for (int r = 0; r < 3; ++r) { const double t = A[r][i]; A[r][i] = A[r][j]; A[r][j] = t; }
    { const double t = y[i]; y[i] = y[j]; y[j] = t; }
    { const int t = perm[i]; perm[i] = perm[j]; perm[j] = t; }
}

// The same solve for a symmetric 3 x 3 A (upper triangle 00 01 02 11 12 22): the colour gradient's normal equations
// (colored.hip).  solve_ldlt6's pivoting, 1e-12 rule and order of operations with 6 read as 3; every array index is a
// constant once the loops are unrolled (the pivot's exchange is chosen by comparisons), so the kernel keeps it in registers.
__host__ __device__ inline bool solve_ldlt3(const double* upper, const double* b, double* x) {
    double A[3][3], y[3];
    int perm[3] = {0, 1, 2};
    for (int r = 0, e = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c, ++e) { A[r][c] = upper[e]; A[c][r] = upper[e]; }
    for (int r = 0; r < 3; ++r) y[r] = b[r];
    double dmax = 0.0;
    // step 0: the largest of the three diagonal entries, the lowest index among equal ones
    if (A[1][1] > A[0][0]) {
        if (A[2][2] > A[1][1]) ldlt3_swap(A, y, perm, 0, 2); else ldlt3_swap(A, y, perm, 0, 1);
    } else if (A[2][2] > A[0][0]) {
        ldlt3_swap(A, y, perm, 0, 2);
    }
    for (int k = 0; k < 3; ++k) {
        if (k == 1 && A[2][2] > A[1][1]) ldlt3_swap(A, y, perm, 1, 2);
        const double d = A[k][k];
        if (d > dmax) dmax = d;
        if (!(d > 1e-12 * dmax) || !(d > 0.0)) return false;
        for (int r = k + 1; r < 3; ++r) A[r][k] = A[r][k] / d;
        for (int r = k + 1; r < 3; ++r)
            for (int c = k + 1; c <= r; ++c) {
                const double v = A[r][c] - A[r][k] * (d * A[c][k]);
                A[r][c] = v;
                A[c][r] = v;
            }
    }
    // L z = y, D w = z, L^T u = w; x[perm] = u
    for (int r = 1; r < 3; ++r)
        for (int c = 0; c < r; ++c) y[r] = y[r] - A[r][c] * y[c];
    for (int r = 0; r < 3; ++r) y[r] = y[r] / A[r][r];
    for (int r = 1; r >= 0; --r)
        for (int c = r + 1; c < 3; ++c) y[r] = y[r] - A[c][r] * y[c];
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 3; ++j)
            if (perm[r] == j) x[j] = y[r];
    return true;
}

}  // namespace
}  // namespace pcrcg
