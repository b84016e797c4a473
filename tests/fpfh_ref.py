"""numpy restatement of the FPFH descriptor (include/pcrcg.h "FPFH descriptors"), brute force, for
tests/test_fpfh_*.py.  The product never imports this file.

Every float64 operation below is one numpy ufunc call, so it rounds once, where the definition says; the order of the
additions is spelled out with brackets."""
import functools

import numpy as np

from . import normals_ref as NR

BINS = 33
EDGE_EPS = 1e-9        # a bin coordinate this close to an interior edge makes the pair fragile
SWAP_EPS = 1e-12       # 0 < ||a1| - |a2|| below this: the swap rule is about to flip
VN_EPS = 1e-12         # 0 < vn <= this * d: dp is all but parallel to n1


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def pair_features(p, n1, q, n2):
    """(p [3], n1 [3]) against m entries (q [m,3], n2 [m,3]), all float64 -> (f [m,3] = (f0, f1, f2), fragile [m] bool)."""
    m = len(q)
    n1 = np.broadcast_to(n1, (m, 3))
    with np.errstate(all="ignore"):
        dp = q - p
        d = np.sqrt(_dot(dp, dp))
        a1 = _dot(n1, dp) / d
        a2 = _dot(n2, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        s3 = swap[:, None]
        m1, m2 = np.where(s3, n2, n1), np.where(s3, n1, n2)
        dp = np.where(s3, -dp, dp)
        f2 = np.where(swap, -a2, a1)
        v = _cross(dp, m1)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = _cross(m1, v)
        f1 = _dot(v, m2)
        f0 = np.arctan2(_dot(w, m2), _dot(m1, m2))
        zero = (d == 0) | (vn == 0)
        f = np.where(zero[:, None], 0.0, np.stack([f0, f1, f2], -1))
        gap = np.abs(np.abs(a1) - np.abs(a2))
        fragile = (d != 0) & (((gap > 0) & (gap < SWAP_EPS)) | ((vn > 0) & (vn <= VN_EPS * d)))
        c = bin_coords(f)
        edge = np.round(c)
        fragile |= ((np.abs(c - edge) < EDGE_EPS) & (edge >= 1) & (edge <= 10)).any(1)
    return f, fragile


def bin_coords(f):
    """f [m,3] -> the three bin coordinates before floor [m,3]."""
    return np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) * 0.5, 11.0 * (f[:, 2] + 1.0) * 0.5], -1)


def histogram(f):
    """f [m,3] -> integer counts [33]; a pair whose f is not all finite counts in no bin."""
    c = np.zeros(BINS, np.int64)
    ok = np.isfinite(f).all(1)
    h = np.clip(np.floor(bin_coords(f[ok])), 0, 10).astype(np.int64)
    for g in range(3):
        np.add.at(c, 11 * g + h[:, g], 1)
    return c


def fpfh(pts, normals, radius, max_nn):
    """The whole definition -> dict: k [n], hist [n,33] int, spfh [n,33], fpfh [n,33] float64, fragile [n] bool (one of the
    point's own pairs is fragile), fragile_any [n] (the point or a member of its list is), nbrs (the lists)."""
    pts = np.asarray(pts, np.float32)
    p64 = pts.astype(np.float64)
    nrm = np.asarray(normals, np.float64)
    n = len(pts)
    nbrs = NR.neighbours(pts, radius, max_nn)
    k = np.array([len(x) for x in nbrs], np.int64)
    hist, spfh, fragile = np.zeros((n, BINS), np.int64), np.zeros((n, BINS)), np.zeros(n, bool)
    for i in range(n):
        if k[i] <= 1:
            continue
        nb = nbrs[i][1:]                                  # entry 0 is skipped, whoever it is
        f, frag = pair_features(p64[i], nrm[i], p64[nb], nrm[nb])
        hist[i] = histogram(f)
        fragile[i] = frag.any()
        spfh[i] = hist[i].astype(np.float64) * (100.0 / (k[i] - 1))
    out = np.zeros((n, BINS))
    fragile_any = fragile.copy()
    for i in range(n):
        if k[i] <= 1:
            continue
        F = np.zeros(BINS)
        for q in nbrs[i][1:]:
            dp = p64[q] - p64[i]
            D = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]
            fragile_any[i] |= fragile[q]
            if D == 0:
                continue
            F = F + spfh[q] / D
        for g in range(3):
            S = 0.0
            for t in range(11):
                S = S + F[11 * g + t]
            if S != 0:
                F[11 * g:11 * g + 11] = F[11 * g:11 * g + 11] * (100.0 / S)
        out[i] = F + spfh[i]
    return {"k": k, "hist": hist, "spfh": spfh, "fpfh": out, "fragile": fragile, "fragile_any": fragile_any, "nbrs": nbrs}


# --- the clouds and normals of the tests -------------------------------------------------------------------------------
def radial_normals(pts, seed, noise=0.1):
    """Unit vectors: the radial direction plus Gaussian noise."""
    p = np.asarray(pts, np.float64)
    v = p / np.linalg.norm(p, axis=1, keepdims=True) + noise * np.random.RandomState(seed).randn(len(p), 3)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def random_normals(n, seed):
    v = np.random.RandomState(seed).randn(n, 3)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


PARITY = {                                              # name -> (cloud, normals, radius); max_nn = 100
    "sphere": lambda: (NR.noisy_sphere(0), radial_normals(NR.noisy_sphere(0), 100), 0.25),
    "cube": lambda: (NR.cube(0), random_normals(1500, 101), 0.15),
    "lattice_sphere": lambda: (NR.lattice_sphere(0), radial_normals(NR.lattice_sphere(0), 102), 0.25),
}


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """-> (pts, normals, radius, reference) of one of the three 1 500-point parity clouds, computed once per process."""
    pts, nrm, r = PARITY[name]()
    return pts, nrm, r, fpfh(pts, nrm, r, 100)


def dense_cube():
    """cube(20, 400): at radius 0.4 up to ~115 points lie in the radius."""
    return NR.cube(20, 400), random_normals(400, 120), 0.4


def height_field(seed=0, n=900):
    """A bumpy height field with no symmetry, coordinates quantised to 2^-10, with the analytic normals of the unquantised
    surface -> (pts f32 [n,3], normals f64 [n,3])."""
    rng = np.random.RandomState(seed)
    xy = rng.rand(n, 2) * 2.0
    x, y = xy[:, 0], xy[:, 1]
    z = 0.3 * np.sin(2.1 * x + 0.3) * np.cos(1.3 * y) + 0.15 * np.sin(3.7 * y + 1.0) + 0.1 * x * y
    zx = 0.3 * 2.1 * np.cos(2.1 * x + 0.3) * np.cos(1.3 * y) + 0.1 * y
    zy = -0.3 * 1.3 * np.sin(2.1 * x + 0.3) * np.sin(1.3 * y) + 0.15 * 3.7 * np.cos(3.7 * y + 1.0) + 0.1 * x
    nrm = np.stack([-zx, -zy, np.ones(n)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = (np.round(np.stack([x, y, z], 1) * 1024.0) / 1024.0).astype(np.float32)
    return pts, nrm


def group_sums(x):
    return np.asarray(x, np.float64).reshape(len(x), 3, 11).sum(2)
