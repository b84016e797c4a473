"""Float64 restatement of the ModelNet evaluation's compute_metrics (ref:lib/tester.py:248-298) in numpy: the oracle
of tests/test_modelnet_metrics_*.py and of scripts/make_golden_modelnet_metrics.py.  Dense [n, m] squared-distance
matrices, nothing clever; it shares no code with pcrcg_amd/modelnet.py."""
import numpy as np

KEYS = ("r_mse", "r_mae", "t_mse", "t_mae", "err_r_deg", "err_t", "chamfer_dist")


def euler_xyz_deg(R):
    """One rotation matrix -> (a, b, c) in degrees with R = Rz(c) Ry(b) Rx(a): scipy's lower-case 'xyz'.  The middle angle
    is taken from the whole first column (atan2), not from R[2,0] alone (asin): on a matrix that is orthonormal only to
    fp32 rounding the two differ by 1e-6 degrees, and so does either from scipy, which normalises a quaternion first."""
    R = np.asarray(R, np.float64)
    b = np.arctan2(-R[2, 0], np.sqrt(R[0, 0] ** 2 + R[1, 0] ** 2))
    if abs(R[2, 0]) > 1.0 - 1e-15:
        return np.degrees(np.array([np.arctan2(-R[1, 2], R[1, 1]), b, 0.0]))
    return np.degrees(np.array([np.arctan2(R[2, 1], R[2, 2]), b, np.arctan2(R[1, 0], R[0, 0])]))


def euler_xyz_matrix(deg):
    """(a, b, c) in degrees -> Rz(c) Ry(b) Rx(a)."""
    a, b, c = np.radians(np.asarray(deg, np.float64))
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rz @ ry @ rx


def _split(T):
    T = np.asarray(T, np.float64)
    return T[:3, :3], T[:3, 3]


def inverse(T):
    R, t = _split(T)
    return np.concatenate([R.T, (R.T @ -t)[:, None]], 1)


def concatenate(A, B):
    Ra, ta = _split(A)
    Rb, tb = _split(B)
    return np.concatenate([Ra @ Rb, (Ra @ tb + ta)[:, None]], 1)


def nearest(queries, candidates):
    """-> (min_j |q_i - c_j|^2 [n], argmin [n], relative gap between the best and the second-best [n]) in float64."""
    q, c = np.asarray(queries, np.float64), np.asarray(candidates, np.float64)
    d = ((q[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    arg = d.argmin(1)
    best = d[np.arange(len(q)), arg]
    if c.shape[0] > 1:
        second = np.partition(d, 1, axis=1)[:, 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.where(second > 0, (second - best) / second, 0.0)
    else:
        gap = np.full(len(q), np.inf)
    return best, arg, gap


def chamfer_pair(points_src, points_ref, points_raw, pred, gt, chunk=1024):
    """One pair -> dict: d_src, arg_src, gap_src, d_ref, arg_ref, gap_ref, mean_src, mean_ref, chamfer (float64)."""
    src, ref, raw = (np.asarray(x, np.float64)[:, :3] for x in (points_src, points_ref, points_raw))
    Rp, tp = _split(pred)
    Rc, tc = _split(concatenate(pred, inverse(gt)))
    moved, clean = src @ Rp.T + tp, raw @ Rc.T + tc
    out = {}
    for side, q, c in (("src", moved, raw), ("ref", ref, clean)):
        parts = [nearest(q[i:i + chunk], c) for i in range(0, len(q), chunk)]
        for k, name in enumerate(("d_", "arg_", "gap_")):
            out[name + side] = np.concatenate([p[k] for p in parts]) if parts else np.zeros(0)
        out["mean_" + side] = out["d_" + side].mean() if len(q) else np.nan
    out["chamfer"] = out["mean_src"] + out["mean_ref"]
    return out


def pose_metrics(gt, pred):
    """One pair -> the six pose-only keys (float64 scalars)."""
    Rg, tg = _split(gt)
    Rp, tp = _split(pred)
    e = euler_xyz_deg(Rg) - euler_xyz_deg(Rp)
    c = concatenate(inverse(gt), pred)
    trace = c[0, 0] + c[1, 1] + c[2, 2]
    return {"r_mse": np.mean(e ** 2), "r_mae": np.mean(np.abs(e)), "t_mse": np.mean((tg - tp) ** 2),
            "t_mae": np.mean(np.abs(tg - tp)),
            "err_r_deg": np.degrees(np.arccos(np.clip(0.5 * (trace - 1.0), -1.0, 1.0))),
            "err_t": np.linalg.norm(c[:, 3])}


def compute_metrics(data, pred_transforms):
    """The reference's compute_metrics pair by pair in float64 -> dict of [B] float64 arrays."""
    B = len(pred_transforms)
    rows = []
    for b in range(B):
        m = pose_metrics(data["transform_gt"][b], pred_transforms[b])
        m["chamfer_dist"] = chamfer_pair(data["points_src"][b], data["points_ref"][b], data["points_raw"][b],
                                         pred_transforms[b], data["transform_gt"][b])["chamfer"]
        rows.append(m)
    return {k: np.array([r[k] for r in rows], np.float64) for k in KEYS}


def summarize_metrics(metrics):
    out = {}
    for k, v in metrics.items():
        v = np.asarray(v, np.float64)
        if k.endswith("mse"):
            out[k[:-3] + "rmse"] = np.sqrt(v.mean())
        elif k.startswith("err"):
            out[k + "_mean"] = v.mean()
            out[k + "_rmse"] = np.sqrt((v ** 2).mean())
        else:
            out[k] = v.mean()
    return out


def fp32_chamfer_pair(points_src, points_ref, points_raw, pred, gt):
    """The reference's FORMULA as a plain fp32 torch run on the CPU (dense matrix, torch.min), written out from
    ref:lib/tester.py:280-286: the yardstick of the fp32 bar.  -> dict: d_src, arg_src, d_ref, arg_ref, mean_src,
    mean_ref, chamfer (numpy)."""
    import torch
    f = lambda x: torch.as_tensor(np.asarray(x)).float()
    src, ref, raw = f(points_src)[None, :, :3], f(points_ref)[None, :, :3], f(points_raw)[None, :, :3]
    P, G = f(pred)[None, :3], f(gt)[None, :3]

    def inv(g):
        r, t = g[..., :3, :3], g[..., :3, 3]
        return torch.cat([r.transpose(-1, -2), r.transpose(-1, -2) @ -t[..., None]], -1)

    def cat(a, b):
        return torch.cat([a[..., :3, :3] @ b[..., :3, :3], a[..., :3, :3] @ b[..., :3, 3:] + a[..., :3, 3:]], -1)

    def move(g, a):
        return a @ g[..., :3, :3].transpose(-1, -2) + g[..., :3, 3][..., None, :]

    def sq(a, b):
        return torch.sum((a[:, :, None, :] - b[:, None, :, :]) ** 2, -1)

    ds, as_ = torch.min(sq(move(P, src), raw), -1)
    dr, ar = torch.min(sq(ref, move(cat(P, inv(G)), raw)), -1)
    ms, mr = torch.mean(ds, 1), torch.mean(dr, 1)
    return {"d_src": ds[0].numpy(), "arg_src": as_[0].numpy(), "d_ref": dr[0].numpy(), "arg_ref": ar[0].numpy(),
            "mean_src": ms[0].numpy(), "mean_ref": mr[0].numpy(), "chamfer": (ms + mr)[0].numpy()}
