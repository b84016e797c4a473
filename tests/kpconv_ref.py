"""Float64 restatement of KPConv.forward in all its configurations (ref:models/blocks.py:229-374), the checker of
tests/test_kpconv_deform_{cpu,gpu}.py, and the recipes of the tensors that tests/golden/kpconv_deform_mini.pt names by
seed.  Plain numpy on the CPU; never the code under test.

The reference is discontinuous where a neighbour sits at distance `extent` from a kernel point (its kept bit flips and
n_q changes by one) and, in 'closest' mode, where two kernel points are equally close.  `fragile_rows` marks the rows that
are within a relative margin of either; comparisons of `out` are made on the other rows."""
import hashlib

import numpy as np

SHADOW = 1e6
K = 15


def digest(t):
    """sha256 of a tensor's / array's bytes (shape and dtype included)."""
    a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t)
    return hashlib.sha256(repr((a.shape, str(a.dtype))).encode() + a.tobytes()).hexdigest()


def normal(seed, shape, scale=1.0):
    """float32 N(0, scale^2) from numpy's legacy generator (its stream is frozen: the same numbers everywhere)."""
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def case_tensors(case):
    """x and the parameters of one fixture case from its recipe: dict(x, weights, [offset_weights, offset_bias])."""
    ns, cin, cout, seed = case["ns"], case["cin"], case["cout"], case["seed"]
    out = {"x": np.ones((ns, 1), np.float32) if cin == 1 else normal(seed, (ns, cin)),
           "weights": normal(seed + 1, (K, cin, cout), 0.2)}
    if case["deformable"] and not case.get("stub_offsets"):      # (the edge cases prescribe offset_features instead)
        od = (4 if case["modulated"] else 3) * K
        out["offset_weights"] = (normal(seed + 2, (K, cin, od)) * np.float32(case["offset_scale"])).astype(np.float32)
        out["offset_bias"] = normal(seed + 3, (od,), 0.08)
    return out


def sq_distances(q_pts, s_pts, idx, kp_q):
    """d2 [nq, H, K] float64 (shadow columns: the point (1e6, 1e6, 1e6)) and real [nq, H]."""
    q = np.asarray(q_pts, np.float64)
    s = np.concatenate([np.asarray(s_pts, np.float64), np.full((1, 3), SHADOW)], 0)
    idx = np.asarray(idx)
    ns = s.shape[0] - 1
    real = (idx >= 0) & (idx < ns)
    nb = s[np.where(real, idx, ns)] - q[:, None, :]
    kp_q = np.asarray(kp_q, np.float64)
    if kp_q.ndim == 2:
        kp_q = np.broadcast_to(kp_q[None], (q.shape[0],) + kp_q.shape)
    diff = nb[:, :, None, :] - kp_q[:, None, :, :]
    return (diff ** 2).sum(-1), real


def deformed_kp(kp, extent, offset_features):
    if offset_features is None:
        return np.asarray(kp, np.float64)
    off = np.asarray(offset_features, np.float64)[:, :3 * K].reshape(-1, K, 3)
    return off * float(extent) + np.asarray(kp, np.float64)[None]


def kept_mask(d2, real, extent, deformable):
    return real & ((d2 < float(extent) ** 2).any(-1) if deformable else True)


def fragile_rows(d2, real, extent, m, deformable, closest):
    """bool [nq]: rows with a real neighbour within m * extent^2 of the kept-set threshold (deformable) or, in closest
    mode, a kept neighbour whose two nearest kernel points are closer than that to a tie."""
    e2 = float(extent) ** 2
    frag = np.zeros(d2.shape[0], bool)
    if deformable:
        frag |= ((np.abs(d2 - e2) < m * e2).any(-1) & real).any(-1)
    if closest:
        two = np.sort(d2, -1)[..., :2]
        frag |= (((two[..., 1] - two[..., 0]) < m * e2) & kept_mask(d2, real, extent, deformable)).any(-1)
    return frag


def fragile_entries(d2, real, extent, m):
    """bool [nq, H]: real neighbours within m * extent^2 of the kept-set threshold."""
    e2 = float(extent) ** 2
    return (np.abs(d2 - e2) < m * e2).any(-1) & real


def kpconv_f64(q_pts, s_pts, idx, x, kp, weights, extent, offset_features=None, influence="linear", aggregation="sum",
               modulated=False):
    """-> dict(out [nq, cout], min_d2 [nq, K], d2, real, kept, n) in float64."""
    extent = float(extent)
    x = np.asarray(x, np.float64)
    deformable = offset_features is not None
    kp_q = deformed_kp(kp, extent, offset_features)
    d2, real = sq_distances(q_pts, s_pts, idx, kp_q)
    kept = kept_mask(d2, real, extent, deformable)
    if influence == "constant":
        w = np.ones_like(d2)
    elif influence == "linear":
        w = np.maximum(1.0 - np.sqrt(d2) / extent, 0.0)
    elif influence == "gaussian":
        w = np.exp(-d2 / (2.0 * (0.3 * extent) ** 2 + 1e-9))
    else:
        raise ValueError(influence)
    if aggregation == "closest":
        w = w * (np.arange(K)[None, None, :] == d2.argmin(-1)[..., None])
    w = w * kept[..., None]
    xs = np.concatenate([x, np.zeros((1, x.shape[1]))], 0)
    nx = xs[np.where(kept, np.asarray(idx), x.shape[0])]                # [nq, H, cin]; not kept -> the zero row
    wf = np.einsum("qhk,qhc->qkc", w, nx)
    if modulated:
        wf = wf * (2.0 / (1.0 + np.exp(-np.asarray(offset_features, np.float64)[:, 3 * K:4 * K])))[..., None]
    out = np.einsum("qkc,kco->qo", wf, np.asarray(weights, np.float64))
    n = np.maximum((nx.sum(-1) > 0).sum(-1), 1)
    return dict(out=out / n[:, None], min_d2=d2.min(1), d2=d2, real=real, kept=kept, n=n, kp_q=kp_q)
