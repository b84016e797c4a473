"""numpy float64 restatement of the robust loss kernels of point-to-plane and colored ICP (include/pcrcg.h "Robust kernels",
csrc/robust_kernel.h, csrc/colored_terms.h colored_terms_robust), for tests/test_robust_*.py: the same
operations in the same order, vectorised over the rows, so that the weights and the 27 weighted terms equal the headers' bit
for bit.  Evaluate(T), the statistics and the convergence test are tests/icp_ref.py's; the 6 x 6 system, its solve and the delta
are tests/icp_plane_ref.py's; sg / sp are tests/colored_icp_ref.py's.  The product never imports this file."""
import numpy as np

from . import colored_icp_ref as CR
from . import icp_plane_ref as PR
from . import icp_ref as IR

L2, L1, HUBER, CAUCHY, GM, TUKEY = range(6)
KINDS = (L2, L1, HUBER, CAUCHY, GM, TUKEY)
NAMES = ("L2", "L1", "Huber", "Cauchy", "GM", "Tukey")
L1_FLOOR = 1e-12            # robust_kernel.h kL1Floor
_UPPER = [(r, c) for r in range(6) for c in range(r, 6)]


def _max(a, b):
    """robust_max: a NaN on either side comes out as a + b, a NaN."""
    return np.where(a >= b, a, np.where(b > a, b, a + b))


def _min(a, b):
    return np.where(a <= b, a, np.where(b < a, b, a + b))


def weight(kind, k, r):
    """robust_weight(kind, k, r) over an array of residuals -> float64 array."""
    r = np.asarray(r, np.float64)
    k = np.float64(k)
    a = np.abs(r)
    one = np.ones_like(r)
    with np.errstate(all="ignore"):
        if kind == L1:
            return one / _max(a, np.float64(L1_FLOOR) * one)
        if kind == HUBER:
            return k / _max(a, k * one)
        if kind == CAUCHY:
            t = r / k
            return one / (one + t * t)
        if kind == GM:
            s = k + r * r
            return k / (s * s)
        if kind == TUKEY:
            t = _min(one, a / k)
            u = one - t * t
            return u * u
        if kind == L2:
            return one
    raise ValueError(kind)


# --- point-to-plane ----------------------------------------------------------------------------------------------------------
def plain_plane_terms_of(p, q, n):
    """The plain estimator's 27 terms of records (k_icp_evaluate<1>'s expressions, written out) -> ([k,27], res [k])."""
    p, q, n = (np.asarray(x, np.float64).reshape(-1, 3) for x in (p, q, n))
    with np.errstate(all="ignore"):
        res = ((p[:, 0] - q[:, 0]) * n[:, 0] + (p[:, 1] - q[:, 1]) * n[:, 1]) + (p[:, 2] - q[:, 2]) * n[:, 2]
        J = [p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
             n[:, 0], n[:, 1], n[:, 2]]
        out = np.empty((len(p), 27))
        for e, (a, b) in enumerate(_UPPER):
            out[:, e] = J[a] * J[b]
        for a in range(6):
            out[:, 21 + a] = -(J[a] * res)
    return out, res


def plane_terms_of(p, q, n, kind, k):
    """plane_terms_robust over records -> [k,27]: w (J_r J_c), then w (-(J_r res)), w = weight(res)."""
    plain, res = plain_plane_terms_of(p, q, n)
    with np.errstate(all="ignore"):
        return weight(kind, k, res)[:, None] * plain


def plane_terms(src, tgt, normals, T, corr, kind, k):
    """The 27 weighted terms of every correspondence of Evaluate(T) -> [count, 27] (icp_plane_ref.terms under a kernel)."""
    corr = np.asarray(corr)
    hit = corr >= 0
    p = IR.move(src, T)[hit].astype(np.float64)
    return plane_terms_of(p, tgt[corr[hit]].astype(np.float64), np.asarray(normals, np.float64)[corr[hit]], kind, k)


# --- colored -----------------------------------------------------------------------------------------------------------------
def colored_terms_of(p, q, rec, Is, sg, sp, kind, k):
    """colored_terms_robust over records -> [k,27]: colored_icp_ref.terms_of's quantities with wg = weight(rg), wi = weight(ri):
    wg (JG_r JG_c) + wi (JI_r JI_c), then -(wg (JG_r rg) + wi (JI_r ri))."""
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
        wg, wi = weight(kind, k, rg), weight(kind, k, ri)
        for e, (r, c) in enumerate(_UPPER):
            out[:, e] = wg * (JG[r] * JG[c]) + wi * (JI[r] * JI[c])
        for r in range(6):
            out[:, 21 + r] = -(wg * (JG[r] * rg) + wi * (JI[r] * ri))
    return out


def colored_terms(src, tgt, rec, src_int, lambda_geometric, T, corr, kind, k):
    """The 27 weighted terms of every correspondence of Evaluate(T) -> [count, 27] (colored_icp_ref.terms under a kernel)."""
    corr = np.asarray(corr)
    hit = corr >= 0
    p = IR.move(src, T)[hit].astype(np.float64)
    sg, sp = CR.weights(lambda_geometric)
    return colored_terms_of(p, tgt[corr[hit]].astype(np.float64), np.asarray(rec, np.float64)[corr[hit]],
                            np.asarray(src_int, np.float64)[hit], sg, sp, kind, k)


# --- what both share: terms [count, 27] -> sums, update, loop -------------------------------------------------------------------
def sums27(terms):
    """-> (the 27 sums, the sums of the (weighted) terms' absolute values)."""
    with np.errstate(all="ignore"):
        return terms.sum(0), np.abs(terms).sum(0)


def update(terms, min_count):
    """-> (delta [4,4] or None when count < min_count (6: point-to-plane, 3: colored), when the weighted system is not finite or
    when the solve refuses it, cond(A) or None).  The count is the number of correspondences: no weight enters it."""
    if len(terms) < min_count:
        return None, None
    with np.errstate(all="ignore"):
        A, b = PR.system(sums27(terms)[0])
        if not np.isfinite(A).all() or not np.isfinite(b).all():
            return None, None
        x = PR.solve_ldlt(A, b)
    if x is None:
        return None, None
    return PR.delta_of(x), float(np.linalg.cond(A))


def icp(src, tgt, T0, d, terms_at, min_count, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """The whole loop with terms_at(T, corr) -> [count, 27] -> (T, fitness, rmse, count, iterations, history); statistics and
    convergence are the plain loop's, unweighted."""
    n = len(src)
    T = np.array(T0, np.float64)
    corr, _, count, total = IR.evaluate(src, tgt, T, d)
    fit, rmse = IR.statistics(count, total, n)
    history = [(T.copy(), fit, rmse)]
    k = 0
    while k < max_iteration:
        delta, _ = update(terms_at(T, corr), min_count)
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


def plane_icp(src, tgt, normals, T0, d, kind, k, **kw):
    return icp(src, tgt, T0, d, lambda T, corr: plane_terms(src, tgt, normals, T, corr, kind, k), PR.MIN_COUNT, **kw)


def colored_icp(src, tgt, rec, src_int, lambda_geometric, T0, d, kind, k, **kw):
    return icp(src, tgt, T0, d, lambda T, corr: colored_terms(src, tgt, rec, src_int, lambda_geometric, T, corr, kind, k),
               CR.MIN_COUNT, **kw)


# --- the outlier scene of tests/test_robust_icp_gpu.py ---------------------------------------------------------------------------
OUTLIER_D, OUTLIER_MI = 0.06, 30
OUTLIER_SCENES = tuple((seed, n) for seed in (0, 1, 2) for n in (600, 1200))


def outlier_scene(seed, n):
    """The corner cloud and its image under the planted pose with a quarter of the targets pushed 0.03 along their normals -- a
    second sheet inside the gate -> src, tgt (float32), the targets' exact normals [n,3], start [4,4], T_gt."""
    T_gt = PR.planted_pose()
    pts = PR.corner(seed, n)
    nrm = PR.corner_normals(pts) @ T_gt[:3, :3].T
    tgt = pts @ T_gt[:3, :3].T + T_gt[:3, 3]
    bad = np.random.RandomState(seed + 50).rand(n) < 0.25
    tgt[bad] += 0.03 * nrm[bad]
    start = PR.delta_of(np.array([0.01, -0.008, 0.012, 0.006, -0.005, 0.007])) @ T_gt
    return pts.astype(np.float32), tgt.astype(np.float32), nrm, start, T_gt
