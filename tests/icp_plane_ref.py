"""numpy restatement of the point-to-plane ICP update (include/pcrcg.h, pcrcg_icp_batch_ex), for
tests/test_icp_plane_*.py.  Evaluate(T), the statistics and the convergence test are tests/icp_ref.py's: the estimators
differ in the update alone.  The product never imports this file."""
import functools

import numpy as np

from . import icp_ref as IR
from . import normals_ref as NR

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


# --- the edge cases of tests/test_icp_plane_edges_gpu.py -----------------------------------------------------------------
def small_pose():
    """Rz(0.005) Ry(-0.003) Rx(0.004), t = (0.01, -0.008, 0.012)."""
    return delta_of(np.array([0.004, -0.003, 0.005, 0.01, -0.008, 0.012]))


LADDER = (0.0, 10.0, 100.0)     # the rungs that update at every step; FAR is refused by the pivot rule at T_0
FAR = 1000.0


def offset_pair(shift, pose=None):
    """The 1 200-point corner cloud and its image under `pose` (small_pose() by default) applied in the cloud's own frame, both
    then moved by `shift` on every axis and rounded to fp32 -> src, tgt, T': the ground truth of the moved pair, T with
    t' = t + s - R s.  J = [p x n, n] is taken about the origin, so A's rotation block grows with shift^2."""
    T = small_pose() if pose is None else np.asarray(pose, np.float64)
    src = corner(0, 1200)
    tgt = src @ T[:3, :3].T + T[:3, 3]
    s = np.full(3, float(shift))
    Ts = T.copy()
    Ts[:3, 3] = T[:3, 3] + s - T[:3, :3] @ s
    return (src + s).astype(np.float32), (tgt + s).astype(np.float32), Ts


LADDER_D, LADDER_R_NORMAL, LADDER_MI = 0.15, 0.12, 10


@functools.lru_cache(maxsize=None)
def ladder_case(shift):
    """offset_pair(shift) with the restated normals of its target (r = 0.12, 30 neighbours) and the restatement's own run from
    the identity (d = 0.15, at most 10 updates) -> src, tgt, T_gt, normals, icp()'s tuple.  Computed once; do not write to it."""
    src, tgt, T_gt = offset_pair(shift)
    nrm = NR.estimate(tgt, LADDER_R_NORMAL, 30)["normals"]
    return src, tgt, T_gt, nrm, icp(src, tgt, nrm, np.eye(4), LADDER_D, max_iteration=LADDER_MI)


def ladder_systems(shift):
    """(A, b) of Evaluate(T_k) at every T_k of the restatement's run on the rung."""
    src, tgt, _, nrm, run = ladder_case(shift)
    return [system(sums27(src, tgt, nrm, Tk, IR.evaluate(src, tgt, Tk, LADDER_D)[0])[0]) for Tk, _, _ in run[5]]


def pivot_ratios(A):
    """The diagonal pivoting of solve_ldlt without its stop rule -> the six pivots, each over the largest so far (fewer when a
    pivot is not positive: that one is the last entry)."""
    A = np.array(A, np.float64)
    out, dmax = [], 0.0
    for k in range(6):
        piv = k
        for r in range(k + 1, 6):
            if A[r, r] > A[piv, piv]:
                piv = r
        if piv != k:
            A[[k, piv], :] = A[[piv, k], :]
            A[:, [k, piv]] = A[:, [piv, k]]
        d = A[k, k]
        dmax = max(dmax, d)
        out.append(d / dmax if dmax > 0 else 0.0)
        if not d > 0.0:
            break
        A[k + 1:, k] = A[k + 1:, k] / d
        for r in range(k + 1, 6):
            for c in range(k + 1, r + 1):
                A[r, c] = A[c, r] = A[r, c] - A[r, k] * (d * A[c, k])
    return np.array(out)


def step_from_sums(s27, T):
    """T_k+1 from the 27 sums of Evaluate(T_k): delta_of(solve_ldlt(A, b)) @ T, or None where the solve refuses."""
    x = solve_ldlt(*system(s27))
    return None if x is None else delta_of(x) @ np.asarray(T, np.float64)


def solve_longdouble(A, b):
    """A x = b by Gaussian elimination with partial pivoting in np.longdouble -> x (np.longdouble)."""
    M = np.concatenate([np.asarray(A, np.longdouble), np.asarray(b, np.longdouble)[:, None]], 1)
    n = len(M)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(M[k:, k])))
        M[[k, piv]] = M[[piv, k]]
        for r in range(k + 1, n):
            M[r] = M[r] - (M[r, k] / M[k, k]) * M[k]
    x = np.zeros(n, np.longdouble)
    for r in range(n - 1, -1, -1):
        x[r] = (M[r, n] - (M[r, r + 1:n] * x[r + 1:]).sum()) / M[r, r]
    return x


def delta_longdouble(x):
    """delta_of in np.longdouble."""
    x = np.asarray(x, np.longdouble)
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    one, zero = np.longdouble(1), np.longdouble(0)
    Rx = np.array([[one, zero, zero], [zero, ca, -sa], [zero, sa, ca]])
    Ry = np.array([[cb, zero, sb], [zero, one, zero], [-sb, zero, cb]])
    Rz = np.array([[cg, -sg, zero], [sg, cg, zero], [zero, zero, one]])
    D = np.eye(4, dtype=np.longdouble)
    D[:3, :3], D[:3, 3] = Rz @ Ry @ Rx, x[3:6]
    return D


def worst_displacement(src, T, T_gt):
    """The largest distance between a source point's image under T and under T_gt (float64)."""
    p = src.astype(np.float64)
    a = p @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]
    b = p @ T_gt[:3, :3].T + T_gt[:3, 3]
    return float(np.sqrt(((a - b) ** 2).sum(1)).max())


def near_plane_pair(n=300, k=8, tilt=2e-3, seed=4):
    """A planar pair that is NOT degenerate by the rule: n points of the plane z = 0 with the normal (0, 0, 1), which fix
    three of the six unknowns, and k points a little off the plane whose exact unit normals lean by `tilt` radians in k
    directions, which fix the other three with a weight of about k tilt^2 / n -> src, tgt, normals, start (plane_pair's)."""
    rng = np.random.RandomState(seed)
    pts = np.concatenate([rng.rand(n, 2), np.zeros((n, 1))], 1)
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))
    phi = 2 * np.pi * (np.arange(k) + 0.25) / k
    off = np.concatenate([rng.rand(k, 2), 0.02 + 0.02 * rng.rand(k, 1)], 1)
    lean = np.stack([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.full(k, np.cos(tilt))], 1)
    pts, nrm = np.concatenate([pts, off]), np.concatenate([nrm, lean])
    start = np.eye(4)
    start[:3, 3] = 0.01 * np.array([0.3, 0.1, 1.0])
    return pts.astype(np.float32), pts.astype(np.float32).copy(), nrm, start


# tilt -> the band of the lowest pivot ratio along the restatement's run: the default pair, and one that a rule of 1e-10
# instead of 1e-12 would refuse (3 x under 1e-10, 30 x over the rule)
NEAR_PLANE_TILTS = {2e-3: (1e-9, 1e-7), 1.5e-4: (1e-11, 1e-10)}

SIZES = (1, 5, 6, 7, 511, 512, 513, 1024, 1025)


def corner_normals(pts):
    """The exact unit normals of corner()'s surface at its own points [n,3] (float64, before any rounding)."""
    n = len(pts)
    face = np.arange(n) % 3
    out = np.zeros((n, 3))
    a = face == 0
    gx = 0.25 * np.cos(5 * pts[a, 0]) * np.cos(4 * pts[a, 1])
    gy = -0.2 * np.sin(5 * pts[a, 0]) * np.sin(4 * pts[a, 1])
    g = np.stack([-gx, -gy, np.ones(a.sum())], 1)
    out[a] = g / np.linalg.norm(g, axis=1, keepdims=True)
    out[face == 1] = [0.0, 1.0, 0.0]
    out[face == 2] = [1.0, 0.0, 0.0]
    return out


def sized_pair(i, n):
    """Pair i of the sizes list: n points of the corner cloud, their n images under the planted pose as targets in another
    order, the targets' exact normals, and a start of its own about 1 degree and 1 cm off the planted pose
    -> src, tgt (float32), normals [n,3] float64, start [4,4]."""
    rng = np.random.RandomState(300 + i)
    T = planted_pose()
    pts = corner(200 + i, n)
    nrm = corner_normals(pts) @ T[:3, :3].T
    order = rng.permutation(n)
    tgt = (pts @ T[:3, :3].T + T[:3, 3])[order]
    off = np.concatenate([np.radians(1.0) * np.array([0.6, -0.5, 0.62]), 0.01 * np.array([0.5, 0.6, -0.62])])
    start = delta_of(off * (1.0 + 0.05 * i)) @ T
    return pts.astype(np.float32), tgt.astype(np.float32), nrm[order], start
