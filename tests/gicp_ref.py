"""numpy float64 restatement of Generalized ICP's update (include/pcrcg.h "Generalized ICP", csrc/gicp_terms.h; DESIGN.md
section 23), for tests/test_gicp_*.py: the same operations in the same order, vectorised over the correspondences, so that its
terms equal the header's bit for bit.  Evaluate(T), the statistics and the convergence test are tests/icp_ref.py's; the
system, the solve and the delta are tests/icp_plane_ref.py's.  The product never imports this file."""
import functools

import numpy as np

from . import icp_plane_ref as PR
from . import icp_ref as IR
from . import normals_ref as NR

MIN_COUNT = 3
PACK = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # (xx, xy, xz, yy, yz, zz)


def covariances_from_normals(normals, epsilon):
    """C = I - (1 - epsilon) n n^T -> [n, 6]: entry (r, c) = (r == c) - ((1 - epsilon) n_r) n_c, each operation rounded."""
    n = np.asarray(normals, np.float64).reshape(-1, 3)
    s = 1.0 - float(epsilon)
    with np.errstate(all="ignore"):
        a = s * n
        return np.stack([(1.0 if r == c else 0.0) - a[:, r] * n[:, c] for r, c in PACK], 1)


def pack(C):
    """[n, 3, 3] -> [n, 6] (the upper triangle)."""
    C = np.asarray(C, np.float64).reshape(-1, 3, 3)
    return np.stack([C[:, r, c] for r, c in PACK], 1)


def unpack(c6):
    """[n, 6] -> [n, 3, 3] symmetric."""
    c6 = np.asarray(c6, np.float64).reshape(-1, 6)
    out = np.empty((len(c6), 3, 3))
    for e, (r, c) in enumerate(PACK):
        out[:, r, c] = out[:, c, r] = c6[:, e]
    return out


def metric_matrix(R, cs, ct):
    """M = C_t + (R C_s) R^T per row -> [n, 6], in the header's order: X = R C_s in full, then the six entries r <= c."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    S = unpack(cs)
    ct = np.asarray(ct, np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        X = np.empty((len(S), 3, 3))
        for r in range(3):
            for c in range(3):
                X[:, r, c] = (R[:, r, 0] * S[:, 0, c] + R[:, r, 1] * S[:, 1, c]) + R[:, r, 2] * S[:, 2, c]
        return np.stack([ct[:, e] + ((X[:, r, 0] * R[:, c, 0] + X[:, r, 1] * R[:, c, 1]) + X[:, r, 2] * R[:, c, 2])
                         for e, (r, c) in enumerate(PACK)], 1)


def adjugate_inverse(m6):
    """W = M^-1 of packed symmetric 3 x 3 matrices [n, 6] -> [n, 6]: six cofactors, det = ((m00 c00 + m01 c01) + m02 c02), six
    divisions.  Nothing is tested: det = 0 or an entry that is not finite gives entries that are not finite."""
    m = np.asarray(m6, np.float64).reshape(-1, 6)
    m00, m01, m02, m11, m12, m22 = (m[:, e] for e in range(6))
    with np.errstate(all="ignore"):
        c00 = m11 * m22 - m12 * m12
        c01 = m02 * m12 - m01 * m22
        c02 = m01 * m12 - m02 * m11
        c11 = m00 * m22 - m02 * m02
        c12 = m01 * m02 - m00 * m12
        c22 = m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        return np.stack([c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det], 1)


def terms_of(p, q, R, cs, ct):
    """The 27 terms of records (p [n,3], q [n,3], R [n,3,3] or [3,3], C_s [n,6], C_t [n,6]) -> [n, 27]: the upper triangle of
    J0^T W J0 row by row, then -J0^T W d, with J0 = [-[p]x | I], d = p - q, W = (C_t + R C_s R^T)^-1."""
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    R = np.broadcast_to(np.asarray(R, np.float64), (len(p), 3, 3))
    w6 = adjugate_inverse(metric_matrix(R, cs, ct))
    W = unpack(w6)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty((len(p), 27))
    with np.errstate(all="ignore"):
        g = np.empty((len(p), 3, 3))
        for r in range(3):
            g[:, r, 0] = py * W[:, r, 2] - pz * W[:, r, 1]
            g[:, r, 1] = pz * W[:, r, 0] - px * W[:, r, 2]
            g[:, r, 2] = px * W[:, r, 1] - py * W[:, r, 0]
        out[:, 0] = py * g[:, 2, 0] - pz * g[:, 1, 0]
        out[:, 1] = py * g[:, 2, 1] - pz * g[:, 1, 1]
        out[:, 2] = py * g[:, 2, 2] - pz * g[:, 1, 2]
        out[:, 3], out[:, 4], out[:, 5] = g[:, 0, 0], g[:, 1, 0], g[:, 2, 0]
        out[:, 6] = pz * g[:, 0, 1] - px * g[:, 2, 1]
        out[:, 7] = pz * g[:, 0, 2] - px * g[:, 2, 2]
        out[:, 8], out[:, 9], out[:, 10] = g[:, 0, 1], g[:, 1, 1], g[:, 2, 1]
        out[:, 11] = px * g[:, 1, 2] - py * g[:, 0, 2]
        out[:, 12], out[:, 13], out[:, 14] = g[:, 0, 2], g[:, 1, 2], g[:, 2, 2]
        out[:, 15:21] = w6
        d0, d1, d2 = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
        e = [(W[:, r, 0] * d0 + W[:, r, 1] * d1) + W[:, r, 2] * d2 for r in range(3)]
        out[:, 21] = -(py * e[2] - pz * e[1])
        out[:, 22] = -(pz * e[0] - px * e[2])
        out[:, 23] = -(px * e[1] - py * e[0])
        out[:, 24], out[:, 25], out[:, 26] = -e[0], -e[1], -e[2]
    return out


def terms(src, tgt, src_cov, tgt_cov, T, corr):
    """The 27 terms of every correspondence of Evaluate(T) -> [count, 27]: p the moved source point (the float64 value of the
    fp32 result), q its target, R the rotation block of T in float64, the source's covariance of the UNMOVED point."""
    corr = np.asarray(corr)
    hit = corr >= 0
    p = IR.move(src, T)[hit].astype(np.float64)
    q = tgt[corr[hit]].astype(np.float64)
    return terms_of(p, q, np.asarray(T, np.float64)[:3, :3], np.asarray(src_cov, np.float64)[hit],
                    np.asarray(tgt_cov, np.float64)[corr[hit]])


def sums27(src, tgt, src_cov, tgt_cov, T, corr):
    """-> (the 27 sums, the sums of the terms' absolute values)."""
    t = terms(src, tgt, src_cov, tgt_cov, T, corr)
    with np.errstate(all="ignore"):
        return t.sum(0), np.abs(t).sum(0)


def update(src, tgt, src_cov, tgt_cov, T, corr):
    """-> (delta [4,4] or None when count < 3 or the solve is refused, cond(A) or None)."""
    if (np.asarray(corr) >= 0).sum() < MIN_COUNT:
        return None, None
    with np.errstate(all="ignore"):
        s, _ = sums27(src, tgt, src_cov, tgt_cov, T, corr)
        A, b = PR.system(s)
        if not np.isfinite(A).all() or not np.isfinite(b).all():
            return None, None
        x = PR.solve_ldlt(A, b)
    if x is None:
        return None, None
    return PR.delta_of(x), float(np.linalg.cond(A))


def icp(src, tgt, src_cov, tgt_cov, T0, d, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """The whole loop -> (T, fitness, rmse, count, iterations, history, conds): history[k] = (T_k, fitness_k, rmse_k), conds[k] =
    cond(A) of the update made at T_k."""
    n = len(src)
    T = np.array(T0, np.float64)
    corr, _, count, total = IR.evaluate(src, tgt, T, d)
    fit, rmse = IR.statistics(count, total, n)
    history, conds = [(T.copy(), fit, rmse)], []
    k = 0
    while k < max_iteration:
        delta, cond = update(src, tgt, src_cov, tgt_cov, T, corr)
        if delta is None:
            break
        conds.append(cond)
        T = delta @ T
        k += 1
        corr, _, count, total = IR.evaluate(src, tgt, T, d)
        fit_prev, rmse_prev = fit, rmse
        fit, rmse = IR.statistics(count, total, n)
        history.append((T.copy(), fit, rmse))
        if IR.converged(fit, rmse, fit_prev, rmse_prev, relative_fitness, relative_rmse):
            break
    return T, fit, rmse, count, k, history, conds


def inverse_longdouble(m6):
    """M^-1 of packed symmetric matrices [n, 6] by the adjugate in np.longdouble -> [n, 6] np.longdouble."""
    m = np.asarray(m6, np.float64).reshape(-1, 6).astype(np.longdouble)
    m00, m01, m02, m11, m12, m22 = (m[:, e] for e in range(6))
    c = [m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11, m00 * m22 - m02 * m02, m01 * m02 - m00 * m12,
         m00 * m11 - m01 * m01]
    det = m00 * c[0] + m01 * c[1] + m02 * c[2]
    return np.stack([x / det for x in c], 1)


# --- the cases of tests/test_gicp_gpu.py (tests/test_gicp_cpu.py checks that they are what they claim) -------------------
D, R_NORMAL, MI, EPSILON = 0.15, 0.12, 10, 1e-3
# The sized pairs take epsilon = 1e-2: five points with discs of 1e-3 give cond(A) = 1.06e4 in this restatement (each point then
# fixes little but its own normal direction), over the 1e4 the cases promise; at 1e-2 the five-point pair has 1.2e3.
SIZED_EPSILON = 1e-2


def _covs(pts, epsilon=EPSILON):
    return covariances_from_normals(NR.estimate(pts, R_NORMAL, 30)["normals"], epsilon)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (src, tgt, C_s [n,6], C_t [m,6], start [4,4], T_gt or None).  Computed once; do not write to it.
      "offset": icp_plane_ref.offset_pair(0), restated normals (r = 0.12 / 30) on both sides, epsilon = 1e-3, from the identity;
      "noisy": corner_pair(0, 1200, 1500, 0.002), the same; "noisy_iso": that pair with identity covariances (epsilon = 1);
      "size<n>": sized_pair(i, n) of icp_plane_ref.SIZES with the surface's exact normals on both sides at SIZED_EPSILON, its
      own start;
      "two", "three": exactly 2 / 3 sources beside targets of their own among 40 scattered ones, scattered normals."""
    if name == "offset":
        src, tgt, T_gt = PR.offset_pair(0)
        return src, tgt, _covs(src), _covs(tgt), np.eye(4), T_gt
    if name in ("noisy", "noisy_iso"):
        src, tgt, T_gt = PR.corner_pair(0, 1200, 1500, 0.002)
        if name == "noisy_iso":
            return src, tgt, covariances_from_normals(np.zeros((1200, 3)), 1.0), covariances_from_normals(np.zeros((1500, 3)), 1.0), \
                np.eye(4), T_gt
        return src, tgt, _covs(src), _covs(tgt), np.eye(4), T_gt
    if name.startswith("size"):
        n = int(name[4:])
        i = PR.SIZES.index(n)
        src, tgt, nrm_t, start = PR.sized_pair(i, n)
        nrm_s = PR.corner_normals(PR.corner(200 + i, n))
        return (src, tgt, covariances_from_normals(nrm_s, SIZED_EPSILON), covariances_from_normals(nrm_t, SIZED_EPSILON), start,
                PR.planted_pose())
    if name in ("two", "three"):
        count = {"two": 2, "three": 3}[name]
        rng = np.random.RandomState(7)
        tgt = (rng.rand(40, 3) * 4.0).astype(np.float32)
        nrm = rng.randn(40 + count, 3)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        src = (tgt[:count].astype(np.float64) + 0.01 * rng.randn(count, 3)).astype(np.float32)
        return src, tgt, covariances_from_normals(nrm[40:], EPSILON), covariances_from_normals(nrm[:40], EPSILON), np.eye(4), None
    raise KeyError(name)


STEP_CASES = ("offset", "noisy") + tuple(f"size{n}" for n in PR.SIZES) + ("two", "three")
