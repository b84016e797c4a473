"""numpy float64 restatement of colored ICP (include/pcrcg.h "Colored ICP", csrc/colored_terms.h, csrc/smallsolve.h
solve_ldlt3), for tests/test_colored_*.py: the same operations in the same order, vectorised over the
rows, so that the gradient rows, the 3 x 3 solve and the 27 terms equal the headers' bit for bit.  The neighbour lists are
tests/normals_ref.py's (brute force, ranked by (d2, index)); Evaluate(T), the statistics and the convergence test are
tests/icp_ref.py's; the 6 x 6 system, its solve and the delta are tests/icp_plane_ref.py's.  The product never imports this
file."""
import functools

import numpy as np

from . import icp_plane_ref as PR
from . import icp_ref as IR
from . import normals_ref as NR

MIN_COUNT = 3               # every correspondence carries two equations
MIN_LIST = 4                # a shorter neighbour list gives no gradient
PIVOT_RATIO = 1e-12
LAMBDA = 0.968              # open3d's default lambda_geometric
_UPPER3 = [(r, c) for r in range(3) for c in range(r, 3)]
_UPPER6 = [(r, c) for r in range(6) for c in range(r, 6)]


def intensity(colors):
    """[n,3] RGB -> ((r + g) + b) / 3.0 in float64; [n] intensities as they are."""
    c = np.asarray(colors, np.float64)
    with np.errstate(all="ignore"):
        return ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0 if c.ndim == 2 else c


# --- the colour gradients ------------------------------------------------------------------------------------------------
def gradient_rows(vt, nt, a, Ia, Ik):
    """The nine products of the rows of one point's fit (colored_terms.h colored_gradient_row): a [k,3] the neighbours, Ia [k]
    their intensities -> [k, 9] = (A0 A0, A0 A1, A0 A2, A1 A1, A1 A2, A2 A2, A0 b, A1 b, A2 b)."""
    vt, nt = np.asarray(vt, np.float64), np.asarray(nt, np.float64)
    a = np.asarray(a, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d0, d1, d2 = a[:, 0] - vt[0], a[:, 1] - vt[1], a[:, 2] - vt[2]
        dot = (d0 * nt[0] + d1 * nt[1]) + d2 * nt[2]
        A = [(a[:, r] - dot * nt[r]) - vt[r] for r in range(3)]
        b = np.asarray(Ia, np.float64) - Ik
        return np.stack([A[r] * A[c] for r, c in _UPPER3] + [A[r] * b for r in range(3)], 1)


def last_row(nt, nn, sums):
    """sums [9] with the fit's last row (nn - 1) nt added to A^T A (colored_gradient_last_row) -> a new [9]."""
    out = np.array(sums, np.float64)
    with np.errstate(all="ignore"):
        r = float(nn - 1) * np.asarray(nt, np.float64)
        for e, (i, j) in enumerate(_UPPER3):
            out[e] = out[e] + r[i] * r[j]
    return out


def solve_ldlt3(upper, b):
    """smallsolve.h solve_ldlt3: icp_plane_ref.solve_ldlt with 6 read as 3 -> x [3], or None where the solve refuses."""
    A = np.zeros((3, 3))
    for e, (r, c) in enumerate(_UPPER3):
        A[r, c] = A[c, r] = upper[e]
    y = np.array(b, np.float64)
    perm = [0, 1, 2]
    dmax = 0.0
    with np.errstate(all="ignore"):
        for k in range(3):
            piv = k
            for r in range(k + 1, 3):
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
            for r in range(k + 1, 3):
                for c in range(k + 1, r + 1):
                    A[r, c] = A[c, r] = A[r, c] - A[r, k] * (d * A[c, k])
        for r in range(1, 3):
            for c in range(r):
                y[r] = y[r] - A[r, c] * y[c]
        for r in range(3):
            y[r] = y[r] / A[r, r]
        for r in range(1, -1, -1):
            for c in range(r + 1, 3):
                y[r] = y[r] - A[c, r] * y[c]
    x = np.zeros(3)
    x[perm] = y
    return x


def pivot_ratios3(upper):
    """The three pivots of solve_ldlt3 without its stop rule, each over the largest so far."""
    A = np.zeros((3, 3))
    for e, (r, c) in enumerate(_UPPER3):
        A[r, c] = A[c, r] = upper[e]
    out, dmax = [], 0.0
    for k in range(3):
        piv = k + int(np.argmax(np.diag(A)[k:]))
        A[[k, piv], :] = A[[piv, k], :]
        A[:, [k, piv]] = A[:, [piv, k]]
        d = A[k, k]
        dmax = max(dmax, d)
        out.append(d / dmax if dmax > 0 else 0.0)
        if not d > 0.0:
            break
        A[k + 1:, k] = A[k + 1:, k] / d
        for r in range(k + 1, 3):
            for c in range(k + 1, r + 1):
                A[r, c] = A[c, r] = A[r, c] - A[r, k] * (d * A[c, k])
    return np.array(out)


def gradients(pts, normals, inten, radius, max_nn):
    """The whole definition for one fp32 cloud -> dict: g [n,3], count [n], sums [n,9] (A^T A's upper triangle then A^T b,
    the last row included; zero where count < 4), mag [n,9] (the sums of the terms' absolute values), solved [n] bool, nbrs."""
    pts = np.asarray(pts, np.float32)
    p64 = pts.astype(np.float64)
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
    inten = np.asarray(inten, np.float64)
    n = len(pts)
    nbrs = NR.neighbours(pts, radius, max_nn)
    g, count, sums, mag = np.zeros((n, 3)), np.zeros(n, np.int64), np.zeros((n, 9)), np.zeros((n, 9))
    solved = np.zeros(n, bool)
    for k, nb in enumerate(nbrs):
        nn = len(nb)
        count[k] = nn
        if nn < MIN_LIST:
            continue
        rows = gradient_rows(p64[k], normals[k], p64[nb[1:]], inten[nb[1:]], inten[k])
        with np.errstate(all="ignore"):
            sums[k] = last_row(normals[k], nn, rows.sum(0))
            mag[k] = last_row(np.abs(normals[k]), nn, np.abs(rows).sum(0))
        x = solve_ldlt3(sums[k, :6], sums[k, 6:])
        if x is not None:
            g[k], solved[k] = x, True
    return {"g": g, "count": count, "sums": sums, "mag": mag, "solved": solved, "nbrs": nbrs}


def records(normals, g, inten):
    """-> [n, 8]: (n [3], g [3], I, 0), the packed rows the update reads."""
    n = len(inten)
    return np.concatenate([np.asarray(normals, np.float64).reshape(n, 3), np.asarray(g, np.float64).reshape(n, 3),
                           np.asarray(inten, np.float64).reshape(n, 1), np.zeros((n, 1))], 1)


# --- the update -------------------------------------------------------------------------------------------------------------
def weights(lambda_geometric):
    """-> sg = sqrt(lambda), sp = sqrt(1 - lambda)."""
    return float(np.sqrt(np.float64(lambda_geometric))), float(np.sqrt(1.0 - np.float64(lambda_geometric)))


def terms_of(p, q, rec, Is, sg, sp):
    """The 27 terms of records (p [k,3], q [k,3], the targets' rec [k,8], the sources' Is [k]) -> [k, 27]
    (colored_terms.h colored_terms): the upper triangle of JG JG^T + JI JI^T row by row, then -(JG rg + JI ri)."""
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    rec = np.asarray(rec, np.float64).reshape(-1, 8)
    Is = np.asarray(Is, np.float64).reshape(-1)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    n0, n1, n2, g0, g1, g2, It = (rec[:, e] for e in range(7))
    out = np.empty((len(p), 27))
    with np.errstate(all="ignore"):
        rG = ((px - q[:, 0]) * n0 + (py - q[:, 1]) * n1) + (pz - q[:, 2]) * n2
        rg = sg * rG
        e0, e1, e2 = (px - rG * n0) - q[:, 0], (py - rG * n1) - q[:, 1], (pz - rG * n2) - q[:, 2]
        I0 = ((g0 * e0 + g1 * e1) + g2 * e2) + It
        ri = sp * (Is - I0)
        gn = (g0 * n0 + g1 * n1) + g2 * n2
        m0, m1, m2 = -(g0 - gn * n0), -(g1 - gn * n1), -(g2 - gn * n2)
        JG = [sg * (py * n2 - pz * n1), sg * (pz * n0 - px * n2), sg * (px * n1 - py * n0), sg * n0, sg * n1, sg * n2]
        JI = [sp * (py * m2 - pz * m1), sp * (pz * m0 - px * m2), sp * (px * m1 - py * m0), sp * m0, sp * m1, sp * m2]
        for e, (r, c) in enumerate(_UPPER6):
            out[:, e] = JG[r] * JG[c] + JI[r] * JI[c]
        for r in range(6):
            out[:, 21 + r] = -(JG[r] * rg + JI[r] * ri)
    return out


def terms(src, tgt, rec, src_int, lambda_geometric, T, corr):
    """The 27 terms of every correspondence of Evaluate(T) -> [count, 27]."""
    corr = np.asarray(corr)
    hit = corr >= 0
    p = IR.move(src, T)[hit].astype(np.float64)
    q = tgt[corr[hit]].astype(np.float64)
    sg, sp = weights(lambda_geometric)
    return terms_of(p, q, np.asarray(rec, np.float64)[corr[hit]], np.asarray(src_int, np.float64)[hit], sg, sp)


def sums27(src, tgt, rec, src_int, lambda_geometric, T, corr):
    """-> (the 27 sums, the sums of the terms' absolute values)."""
    t = terms(src, tgt, rec, src_int, lambda_geometric, T, corr)
    with np.errstate(all="ignore"):
        return t.sum(0), np.abs(t).sum(0)


def update(src, tgt, rec, src_int, lambda_geometric, T, corr):
    """-> (delta [4,4] or None when count < 3 or the solve is refused, cond(A) or None)."""
    if (np.asarray(corr) >= 0).sum() < MIN_COUNT:
        return None, None
    with np.errstate(all="ignore"):
        s, _ = sums27(src, tgt, rec, src_int, lambda_geometric, T, corr)
        A, b = PR.system(s)
        if not np.isfinite(A).all() or not np.isfinite(b).all():
            return None, None
        x = PR.solve_ldlt(A, b)
    if x is None:
        return None, None
    return PR.delta_of(x), float(np.linalg.cond(A))


def icp(src, tgt, rec, src_int, lambda_geometric, T0, d, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """The whole loop -> (T, fitness, rmse, count, iterations, history, conds): history[k] = (T_k, fitness_k, rmse_k), conds[k] =
    cond(A) of the update made at T_k."""
    n = len(src)
    T = np.array(T0, np.float64)
    corr, _, count, total = IR.evaluate(src, tgt, T, d)
    fit, rmse = IR.statistics(count, total, n)
    history, conds = [(T.copy(), fit, rmse)], []
    k = 0
    while k < max_iteration:
        delta, cond = update(src, tgt, rec, src_int, lambda_geometric, T, corr)
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


# --- the cases of tests/test_colored_icp_gpu.py (tests/test_colored_icp_cpu.py checks that they are what they claim) -----------
D, MI = 0.15, 10
R_GRADIENT, NN_GRADIENT = 2 * D, 30


def texture(pts):
    """A smooth colour field on points in their own (source) frame -> [n,3] RGB in [0, 1]: wavelengths of a unit and more, far
    above every planted displacement."""
    x, y, z = (np.asarray(pts, np.float64)[:, e] for e in range(3))
    return np.stack([0.5 + 0.3 * np.sin(4.0 * x + 0.5) * np.cos(3.0 * y), 0.5 + 0.3 * np.cos(3.5 * y - 0.4 * z) * np.sin(2.0 * x + 1.0),
                     0.5 + 0.2 * np.sin(3.0 * z + 2.0 * x) + 0.2 * np.cos(2.5 * y)], 1)


def plane_pose():
    """The planted in-plane pose of the textured plane: Rz(0.05) about the origin, t = (0.05, -0.04, 0)."""
    return PR.delta_of(np.array([0.0, 0.0, 0.05, 0.05, -0.04, 0.0]))


def textured_plane(n, m=400, seed=12):
    """n sources and m independent targets on the unit square of the plane z = 0, the targets under plane_pose(), colours the
    texture at the points' own coordinates, exact normals (0, 0, 1) -> src, tgt (float32), src RGB, tgt RGB, normals, T_gt.
    Geometry says nothing about the in-plane pose: point-to-plane's system is singular here."""
    rng = np.random.RandomState(seed + n)
    T = plane_pose()
    ps = np.concatenate([rng.rand(n, 2), np.zeros((n, 1))], 1)
    pt = np.concatenate([rng.rand(m, 2), np.zeros((m, 1))], 1)
    tgt = pt @ T[:3, :3].T + T[:3, 3]
    return ps.astype(np.float32), tgt.astype(np.float32), texture(ps), texture(pt), np.tile([0.0, 0.0, 1.0], (m, 1)), T


PLANES = (300, 7, 513)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (src, tgt, src RGB, tgt RGB, tgt normals [m,3], start [4,4], T_gt or None, rec [m,8], src_int [n]): the last two
    are the restated records (gradients at R_GRADIENT / NN_GRADIENT) and intensities.  Computed once; do not write to it.
      "plane<n>": textured_plane(n) from the identity;
      "size<n>": icp_plane_ref.sized_pair(i, n) of icp_plane_ref.SIZES with the texture on its surface, its own start."""
    if name.startswith("plane"):
        src, tgt, cs, ct, nrm, T_gt = textured_plane(int(name[5:]))
        start = np.eye(4)
    elif name.startswith("size"):
        n = int(name[4:])
        i = PR.SIZES.index(n)
        src, tgt, nrm, start = PR.sized_pair(i, n)
        col = texture(PR.corner(200 + i, n))
        cs, ct, T_gt = col, col[np.random.RandomState(300 + i).permutation(n)], PR.planted_pose()
    else:
        raise KeyError(name)
    it = intensity(ct)
    rec = records(nrm, gradients(tgt, nrm, it, R_GRADIENT, NN_GRADIENT)["g"], it)
    return src, tgt, cs, ct, nrm, start, T_gt, rec, intensity(cs)


STEP_CASES = tuple(f"size{n}" for n in PR.SIZES) + tuple(f"plane{n}" for n in PLANES)
