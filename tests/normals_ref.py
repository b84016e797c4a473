"""numpy restatement of the normal estimation (include/pcrcg.h "Normal estimation"), brute force, for
tests/test_normals_*.py.  The product never imports this file."""
import numpy as np


def neighbours(pts, radius, max_nn):
    """-> list of int64 arrays: for every point of the fp32 cloud pts [n,3], the points with d2 < (float)r * (float)r
    (d2 = ((dx dx + dy dy) + dz dz) in fp32, the point itself among them) in ascending (d2, index) order, cut to max_nn."""
    pts = np.asarray(pts, np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    out = []
    for i in range(len(pts)):
        dx, dy, dz = pts[:, 0] - pts[i, 0], pts[:, 1] - pts[i, 1], pts[:, 2] - pts[i, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        idx = np.flatnonzero(d2 < r2)
        order = np.lexsort((idx, d2[idx]))              # d2 first, then the index
        out.append(idx[order][:max_nn].astype(np.int64))
    return out


def moments(pts, nbrs):
    """-> (count [n] int, cov [n,6] float64 = (xx, xy, xz, yy, yz, zz) of C = sum d d^T / k - m m^T about the query point,
    scale [n] = sum |d|^2 / k: what the covariance's rounding error is measured against)."""
    p64 = np.asarray(pts, np.float32).astype(np.float64)
    n = len(p64)
    count, cov, scale = np.zeros(n, np.int64), np.zeros((n, 6)), np.zeros(n)
    for i, nb in enumerate(nbrs):
        k = len(nb)
        count[i] = k
        if k == 0:
            continue
        d = p64[nb] - p64[i]
        m = d.sum(0) / k
        S = (d[:, :, None] * d[:, None, :]).sum(0) / k
        C = S - np.outer(m, m)
        cov[i] = C[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
        scale[i] = (d * d).sum() / k
    return count, cov, scale


def as_matrix(c):
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])


def orient(n, p, viewpoint):
    """The sign rule: n . (v - p) >= 0; on the plane through the viewpoint the first non-zero component is positive."""
    dot = (n[0] * (viewpoint[0] - p[0]) + n[1] * (viewpoint[1] - p[1])) + n[2] * (viewpoint[2] - p[2])
    lead = n[np.flatnonzero(n)[0]] if np.any(n != 0) else 0.0
    return -n if dot < 0 or (dot == 0 and lead < 0) else n


def sign_ok(n, p, viewpoint):
    return np.array_equal(orient(np.asarray(n, np.float64), np.asarray(p, np.float64), np.asarray(viewpoint, np.float64)), n)


def estimate(pts, radius, max_nn, viewpoint=None):
    """The whole definition -> dict: normals [n,3] float64, count [n], cov [n,6], scale [n], eig [n,3] (ascending eigenvalues
    of C, np.linalg.eigh), fallback [n] bool (count < 3 or C identically zero: the row is (0, 0, 1), not oriented)."""
    pts = np.asarray(pts, np.float32)
    v = np.zeros(3) if viewpoint is None else np.asarray(viewpoint, np.float64)
    nbrs = neighbours(pts, radius, max_nn)
    count, cov, scale = moments(pts, nbrs)
    n = len(pts)
    normals, eig, fallback = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, bool)
    for i in range(n):
        if count[i] < 3 or not cov[i].any():
            normals[i] = (0.0, 0.0, 1.0)
            fallback[i] = True
            continue
        w, V = np.linalg.eigh(as_matrix(cov[i]))
        eig[i] = w
        normals[i] = orient(V[:, 0] / np.linalg.norm(V[:, 0]), pts[i].astype(np.float64), v)
    return {"normals": normals, "count": count, "cov": cov, "scale": scale, "eig": eig, "fallback": fallback, "nbrs": nbrs}


def well_separated(eig, gap=1e-3):
    """Rows whose smallest eigenvalue is separated from the next by gap times the largest: (l1 - l0) / l2 >= gap."""
    l2 = np.where(eig[:, 2] > 0, eig[:, 2], 1.0)
    return (eig[:, 2] > 0) & ((eig[:, 1] - eig[:, 0]) / l2 >= gap)


# --- the clouds of the tests -------------------------------------------------------------------------------------------
def noisy_sphere(seed, n=1500, noise=0.01):
    rng = np.random.RandomState(seed)
    u = rng.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * (1.0 + noise * rng.randn(n, 1))).astype(np.float32)


def cube(seed, n=1500):
    return np.random.RandomState(seed).rand(n, 3).astype(np.float32)


def lattice_sphere(seed, n=1500, h=0.02):
    """The noisy sphere snapped to a lattice of spacing h: many equal distances, and coincident points."""
    return (np.round(noisy_sphere(seed, n).astype(np.float64) / h) * h).astype(np.float32)


def tie_lattice(seed, k=5, h=0.125):
    """A k^3 lattice of spacing h (a power of two: every d2 is exact in fp32) in a random index order: with radius 1.5 h an
    interior point has itself, 6 neighbours at h^2 and 12 at 2 h^2, so a cut at max_nn = 4 or 10 falls inside a group of
    equal d2 and the index order decides."""
    rng = np.random.RandomState(seed)
    ijk = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 3)
    return (ijk[rng.permutation(len(ijk))] * h).astype(np.float32)
