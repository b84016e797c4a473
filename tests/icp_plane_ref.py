"""numpy restatement of the point-to-plane ICP update (include/pcrcg.h, pcrcg_icp_batch_ex), for
tests/test_icp_plane_*.py.  Evaluate(T), the statistics and the convergence test are tests/icp_ref.py's: the estimators
differ in the update alone.  The product never imports this file."""
import numpy as np

from . import icp_ref as IR

MIN_COUNT = 6
PIVOT_RATIO = 1e-12
_UPPER = [(r, c) for r in range(6) for c in range(r, 6)]


def terms(src, tgt, normals, T, corr):
    """The 27 terms of every correspondence of Evaluate(T) -> [count, 27] float64: J J^T's upper triangle row by row, then
    -J r, with p the moved source point (the float64 value of the fp32 result), q its target, n the target's normal,
    r = (p - q) . n and J = [p x n, n]."""
    hit = corr >= 0
    p = IR.move(src, T)[hit].astype(np.float64)
    q = tgt[corr[hit]].astype(np.float64)
    n = np.asarray(normals, np.float64)[corr[hit]]
    r = ((p[:, 0] - q[:, 0]) * n[:, 0] + (p[:, 1] - q[:, 1]) * n[:, 1]) + (p[:, 2] - q[:, 2]) * n[:, 2]
    J = np.concatenate([np.cross(p, n), n], 1)
    out = np.empty((len(p), 27))
    for e, (a, b) in enumerate(_UPPER):
        out[:, e] = J[:, a] * J[:, b]
    out[:, 21:] = -(J * r[:, None])
    return out


def sums27(src, tgt, normals, T, corr):
    """-> (the 27 sums, the sums of the terms' absolute values)."""
    t = terms(src, tgt, normals, T, corr)
    return t.sum(0), np.abs(t).sum(0)


def system(s27):
    A = np.zeros((6, 6))
    for e, (a, b) in enumerate(_UPPER):
        A[a, b] = A[b, a] = s27[e]
    return A, np.array(s27[21:27], np.float64)


def solve_ldlt(A, b):
    """A x = b by LDL^T with diagonal pivoting (the largest remaining diagonal entry, the lowest index among equal ones) ->
    x, or None as soon as a pivot is not above PIVOT_RATIO times the largest pivot so far."""
    A = np.array(A, np.float64)
    y = np.array(b, np.float64)
    perm = list(range(6))
    dmax = 0.0
    for k in range(6):
        piv = k
        for r in range(k + 1, 6):
            if A[r, r] > A[piv, piv]:
                piv = r
        if piv != k:
            A[[k, piv], :] = A[[piv, k], :]
            A[:, [k, piv]] = A[:, [piv, k]]
            y[[k, piv]] = y[[piv, k]]
            perm[k], perm[piv] = perm[piv], perm[k]
        d = A[k, k]
        if d > dmax:
            dmax = d
        if not (d > PIVOT_RATIO * dmax) or not (d > 0.0):
            return None
        A[k + 1:, k] = A[k + 1:, k] / d
        for r in range(k + 1, 6):
            for c in range(k + 1, r + 1):
                A[r, c] = A[c, r] = A[r, c] - A[r, k] * (d * A[c, k])
    for r in range(1, 6):
        for c in range(r):
            y[r] -= A[r, c] * y[c]
    y /= np.diag(A)
    for r in range(4, -1, -1):
        for c in range(r + 1, 6):
            y[r] -= A[c, r] * y[c]
    x = np.zeros(6)
    x[perm] = y
    return x


def delta_of(x):
    """open3d's TransformVector6dToMatrix4d: Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = Rz @ Ry @ Rx, x[3:6]
    return D


def update(src, tgt, normals, T, corr):
    """-> (delta [4,4] or None when count < 6 or the system is degenerate, cond(A) or None)."""
    if (corr >= 0).sum() < MIN_COUNT:
        return None, None
    with np.errstate(all="ignore"):
        s, _ = sums27(src, tgt, normals, T, corr)
        A, b = system(s)
        if not np.isfinite(A).all() or not np.isfinite(b).all():
            return None, None
        x = solve_ldlt(A, b)
    if x is None:
        return None, None
    return delta_of(x), float(np.linalg.cond(A))


def icp(src, tgt, normals, T0, d, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """The whole loop -> (T, fitness, rmse, count, iterations, history): history[k] = (T_k, fitness_k, rmse_k)."""
    n = len(src)
    T = np.array(T0, np.float64)
    corr, _, count, total = IR.evaluate(src, tgt, T, d)
    fit, rmse = IR.statistics(count, total, n)
    history = [(T.copy(), fit, rmse)]
    k = 0
    while k < max_iteration:
        delta, _ = update(src, tgt, normals, T, corr)
        if delta is None:
            break
        T = delta @ T
        k += 1
        corr, _, count, total = IR.evaluate(src, tgt, T, d)
        fit_prev, rmse_prev = fit, rmse
        fit, rmse = IR.statistics(count, total, n)
        history.append((T.copy(), fit, rmse))
        if IR.converged(fit, rmse, fit_prev, rmse_prev, relative_fitness, relative_rmse):
            break
    return T, fit, rmse, count, k, history


# --- the clouds of the tests -------------------------------------------------------------------------------------------
def planted_pose():
    """Rz(0.08) Ry(-0.05) Rx(0.06), t = (0.03, -0.02, 0.04)."""
    return delta_of(np.array([0.06, -0.05, 0.08, 0.03, -0.02, 0.04]))


def corner(seed, n):
    """n points (n / 3 per face) on the unit squares of the three coordinate planes, the z = 0 face waved by
    0.05 sin 5x cos 4y -> float64 [n,3]."""
    rng = np.random.RandomState(seed)
    u = rng.rand(n, 2)
    face = np.arange(n) % 3
    pts = np.zeros((n, 3))
    a = face == 0
    pts[a, 0], pts[a, 1] = u[a, 0], u[a, 1]
    pts[a, 2] = 0.05 * np.sin(5 * u[a, 0]) * np.cos(4 * u[a, 1])
    b = face == 1
    pts[b, 0], pts[b, 2] = u[b, 0], u[b, 1]
    c = face == 2
    pts[c, 1], pts[c, 2] = u[c, 0], u[c, 1]
    return pts


def corner_pair(seed=0, n=1200, m=None, noise=0.0):
    """-> src, tgt (float32), T_gt: the corner cloud and its image under the planted pose; with m, the target is an
    independent sample of m points of the same surface, with Gaussian noise."""
    T = planted_pose()
    src = corner(seed, n)
    base = src if m is None else corner(seed + 1000, m)
    rng = np.random.RandomState(seed + 2000)
    tgt = base @ T[:3, :3].T + T[:3, 3] + noise * rng.randn(*base.shape)
    return src.astype(np.float32), tgt.astype(np.float32), T


def plane_pair(tilted, n=300, seed=3):
    """A planar pair with exact normals: z = 0, or the same plane rotated about a skew axis -> src, tgt, normals, start."""
    rng = np.random.RandomState(seed)
    pts = np.concatenate([rng.rand(n, 2), np.zeros((n, 1))], 1)
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))
    if tilted:
        R = delta_of(np.array([0.4, -0.3, 0.2, 0, 0, 0]))[:3, :3]
        pts, nrm = pts @ R.T + np.array([0.1, 0.2, 0.3]), nrm @ R.T
    start = np.eye(4)
    start[:3, 3] = 0.01 * (nrm[0] + np.array([0.3, 0.1, 0.0]))
    return pts.astype(np.float32), pts.astype(np.float32).copy(), nrm, start
