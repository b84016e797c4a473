"""ModelNet / ModelLoNet evaluation: what ModelnetTester computes from the estimated poses (ref:lib/tester.py:248-334).

  * `chamfer_batch`     -- the modified Chamfer distance of B ragged pairs in ONE call of pcrcg_chamfer_batch
                           (csrc/chamfer.hip; include/pcrcg.h has the arithmetic contract) -> `ChamferResult`.
  * `compute_metrics`   -- the reference's signature and result keys for B >= 1 pairs in one call: the six pose-only
                           metrics on the host in float64, `chamfer_dist` from `chamfer_batch`.
  * `summarize_metrics` -- ref:lib/tester.py:322-334.
  * `dcm2euler_xyz`     -- rotation matrices -> Euler angles in scipy's lower-case 'xyz' convention, in numpy.
  * `print_metrics`     -- the reference's report lines.

The reference computes the pose-only metrics in fp32; near a zero residual rotation its `err_r_deg` (the arc cosine of an
fp32 trace) is rounding noise.  Here they are float64 functions of the given matrices.  scipy is not needed: the
reference's `Rotation.from_dcm(...).as_euler('xyz')` is restated in `dcm2euler_xyz`.
"""
import numpy as np
import torch

from . import _lib, ragged

# calls of pcrcg_chamfer_batch made by this module (tests count them: one per chamfer_batch / compute_metrics call)
CALLS = [0]

METRIC_KEYS = ("r_mse", "r_mae", "t_mse", "t_mae", "err_r_deg", "err_t", "chamfer_dist")


class ChamferResult:
    """Results of `chamfer_batch` for B pairs, numpy from the one read: chamfer, mean_src, mean_ref float32 [B]
    (chamfer = mean_src + mean_ref, NaN for a pair with an empty cloud) and n_src, n_ref, n_raw int64 [B].  With
    per_point=True also lists of per-pair arrays: d_src [n_b] / d_ref [m_b] float32, the nearest squared distances, and
    arg_src / arg_ref int64, the index of the nearest candidate in the pair's points_raw (lowest on ties, -1 where the
    distance is NaN); None otherwise."""

    def __init__(self, ns, ms, rs, chamfer, mean_src, mean_ref, d_src=None, arg_src=None, d_ref=None, arg_ref=None):
        self.n_src, self.n_ref, self.n_raw = (np.asarray(x, dtype=np.int64) for x in (ns, ms, rs))
        self.chamfer, self.mean_src, self.mean_ref = chamfer, mean_src, mean_ref
        self.d_src, self.arg_src, self.d_ref, self.arg_ref = d_src, arg_src, d_ref, arg_ref

    def __len__(self):
        return len(self.chamfer)

    def __repr__(self):
        return f"ChamferResult(pairs={len(self)}, mean chamfer={float(np.nanmean(self.chamfer)):.6g})"


def _cloud_list(x, name):
    """A [B, n, 3] tensor / array or a list of [n_b, >= 3] clouds -> list of per-pair clouds (columns :3 taken later)."""
    if isinstance(x, (torch.Tensor, np.ndarray)):
        if x.ndim != 3:
            raise ValueError(f"chamfer_batch: {name} must be a [B, n, 3] array or a list of [n_b, 3] arrays, got {tuple(x.shape)}")
        return list(x)
    return list(x)


def _stack_clouds(xs, dev, name):
    ts = ragged.tensors(xs)
    for b, t in enumerate(ts):
        if t.dim() != 2 or t.shape[1] < 3:
            raise ValueError(f"chamfer_batch: {name}[{b}] must be [n, 3], got {tuple(t.shape)}")
    return ragged.join(ts, dev, torch.float32, lambda t: t[:, :3])


def _poses(x, B, dev, name):
    """[B, 3|4, 4] poses (tensor, array or list) -> [B, 12] float32 device tensor, R row-major then t."""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        x = np.stack([t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in x])
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dim() != 3 or t.shape[0] != B or t.shape[1] not in (3, 4) or t.shape[2] != 4:
        raise ValueError(f"chamfer_batch: {name} must be [{B}, 3|4, 4], got {tuple(t.shape)}")
    t = t.to(device=dev, dtype=torch.float32)
    return torch.cat([t[:, :3, :3].reshape(B, 9), t[:, :3, 3]], 1).contiguous()


def chamfer_batch(points_src, points_ref, points_raw, pred, gt, *, per_point=False):
    """compute_metrics' modified Chamfer distance (ref:lib/tester.py:280-286) for B pairs in ONE call of
    pcrcg_chamfer_batch -> ChamferResult.  For pair b: d_src = the squared distance of every row of pred_b * points_src_b to
    its nearest row of points_raw_b, d_ref = that of every row of points_ref_b to (pred_b o gt_b^-1) * points_raw_b, chamfer
    = mean(d_src) + mean(d_ref).

    points_*: lists of ragged [n_b, 3] clouds or [B, n, 3] arrays (torch on the device or the host, or numpy; further
    columns such as normals are ignored, as the reference's `[..., :3]`); pred, gt: [B, 3|4, 4].  Sizes are checked on
    the host before anything is uploaded or launched; the result is read from the device once.  A pair's values do not
    depend on the other pairs of the call (bit for bit)."""
    src, ref, raw = (_cloud_list(x, n) for x, n in ((points_src, "points_src"), (points_ref, "points_ref"),
                                                     (points_raw, "points_raw")))
    B = len(src)
    if B == 0:
        raise ValueError("chamfer_batch: no pairs")
    if not len(ref) == len(raw) == B:
        raise ValueError(f"chamfer_batch: list lengths differ ({B}, {len(ref)}, {len(raw)})")
    if B > ragged.MAX_BATCH:
        raise ValueError(f"chamfer_batch: {B} pairs, one call takes up to {ragged.MAX_BATCH}")
    ns, ms, rs = ([ragged.rows(x) for x in xs] for xs in (src, ref, raw))
    N, M, R = sum(ns), sum(ms), sum(rs)
    if max(N, M, R) > ragged.MAX_ROWS:
        raise ValueError("chamfer_batch: more than 2^31 - 1 rows in one call")
    dev = ragged.device([*src, *ref, *raw], "registration")
    P, G = _poses(pred, B, dev, "pred"), _poses(gt, B, dev, "gt")
    s, r, w = _stack_clouds(src, dev, "points_src"), _stack_clouds(ref, dev, "points_ref"), _stack_clouds(raw, dev, "points_raw")
    off_s, off_r, off_w = ragged.offsets(dev, ns, ms, rs)
    L = _lib.lib()
    wsb = L.pcrcg_chamfer_batch_ws_bytes(B, N, M, R)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    # one int32 buffer, read once: chamfer | mean_src | mean_ref [B] (f32 bits) | d_src [N] | arg_src [N] | d_ref [M] | arg_ref [M]
    o_ds = 3 * B
    o_as, o_dr, o_ar = o_ds + N, o_ds + 2 * N, o_ds + 2 * N + M
    out = torch.empty(3 * B + (2 * (N + M) if per_point else 0), dtype=torch.int32, device=dev)

    def ptr(t, o=0, on=True):
        # an empty stack still needs a pointer the entry accepts; nothing is read through it
        return (t[o:].data_ptr() if t.numel() > o else out.data_ptr()) if on else None

    _lib.check(L.pcrcg_chamfer_batch(ptr(s), off_s.data_ptr(), N, ptr(r), off_r.data_ptr(), M, ptr(w),
                                     off_w.data_ptr(), R, B, P.data_ptr(), G.data_ptr(), out.data_ptr(),
                                     out[B:].data_ptr(), out[2 * B:].data_ptr(), ptr(out, o_ds, per_point),
                                     ptr(out, o_as, per_point), ptr(out, o_dr, per_point), ptr(out, o_ar, per_point),
                                     ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream), "pcrcg_chamfer_batch")
    CALLS[0] += 1
    h = ragged.read(out)
    f = h[:3 * B].view(np.float32).reshape(3, B).copy()
    extra = ()
    if per_point:
        cn, cm = np.cumsum(ns)[:-1], np.cumsum(ms)[:-1]
        extra = (np.split(h[o_ds:o_as].view(np.float32).copy(), cn), np.split(h[o_as:o_dr].astype(np.int64), cn),
                 np.split(h[o_dr:o_ar].view(np.float32).copy(), cm), np.split(h[o_ar:o_ar + M].astype(np.int64), cm))
    return ChamferResult(ns, ms, rs, f[0], f[1], f[2], *extra)


def dcm2euler_xyz(mats, degrees=True):
    """Rotation matrices [B, 3, 3] -> Euler angles [B, 3] float64 in scipy's lower-case 'xyz' convention (extrinsic
    rotations about x, then y, then z: R = Rz(c) Ry(b) Rx(a), returned as (a, b, c)), what the reference's
    dcm2euler(..., seq='xyz') returns.  b lies in [-90, 90] degrees.  In the gimbal case |R[2,0]| = 1 only a -+ c is
    determined: c is set to 0, as scipy does."""
    R = np.asarray(mats, dtype=np.float64).reshape(-1, 3, 3)
    cb = np.hypot(R[:, 0, 0], R[:, 1, 0])
    b = np.arctan2(-R[:, 2, 0], cb)
    lock = cb < 1e-12
    a = np.where(lock, np.arctan2(-R[:, 1, 2], R[:, 1, 1]), np.arctan2(R[:, 2, 1], R[:, 2, 2]))
    c = np.where(lock, 0.0, np.arctan2(R[:, 1, 0], R[:, 0, 0]))
    out = np.stack([a, b, c], 1)
    return np.degrees(out) if degrees else out


def _poses_f64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    elif not isinstance(x, np.ndarray):
        x = np.stack([t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in x])
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3 or x.shape[1] not in (3, 4) or x.shape[2] != 4:
        raise ValueError(f"compute_metrics: transforms must be [B, 3|4, 4], got {x.shape}")
    return x[:, :3, :]


def pose_metrics(gt_transforms, pred_transforms):
    """The six pose-only keys of compute_metrics (ref:lib/tester.py:262-278) in float64 numpy, [B] each: mean squared /
    absolute difference of the 'xyz' Euler angles in degrees (r_mse, r_mae) and of the translations (t_mse, t_mae), and
    the isotropic errors of gt^-1 o pred: err_r_deg = acos(clamp((trace - 1) / 2, -1, 1)) in degrees, err_t = |t|."""
    G, P = _poses_f64(gt_transforms), _poses_f64(pred_transforms)
    if G.shape != P.shape:
        raise ValueError(f"compute_metrics: {G.shape[0]} ground-truth and {P.shape[0]} predicted transforms")
    e = dcm2euler_xyz(G[:, :, :3]) - dcm2euler_xyz(P[:, :, :3])
    dt = G[:, :, 3] - P[:, :, 3]
    Rg_t = np.transpose(G[:, :, :3], (0, 2, 1))
    Rc = Rg_t @ P[:, :, :3]
    tc = (Rg_t @ P[:, :, 3:])[..., 0] + (Rg_t @ -G[:, :, 3:])[..., 0]
    trace = Rc[:, 0, 0] + Rc[:, 1, 1] + Rc[:, 2, 2]
    return {
        "r_mse": np.mean(e ** 2, axis=1),
        "r_mae": np.mean(np.abs(e), axis=1),
        "t_mse": np.mean(dt ** 2, axis=1),
        "t_mae": np.mean(np.abs(dt), axis=1),
        "err_r_deg": np.degrees(np.arccos(np.clip(0.5 * (trace - 1.0), -1.0, 1.0))),
        "err_t": np.linalg.norm(tc, axis=1),
    }


def compute_metrics(data, pred_transforms):
    """ref:lib/tester.py:248-298 for B >= 1 pairs in ONE call -> dict of numpy [B] arrays under the reference's keys
    (r_mse, r_mae, t_mse, t_mae, err_r_deg, err_t: float64, computed on the host; chamfer_dist: float32, from
    chamfer_batch).  data: 'transform_gt' [B, 3|4, 4] and 'points_src', 'points_ref', 'points_raw' ([B, n, >= 3] arrays
    or lists of ragged [n_b, >= 3] clouds; columns :3 are used); pred_transforms: [B, 3|4, 4]."""
    metrics = pose_metrics(data["transform_gt"], pred_transforms)
    metrics["chamfer_dist"] = chamfer_batch(data["points_src"], data["points_ref"], data["points_raw"], pred_transforms,
                                            data["transform_gt"]).chamfer
    return metrics


def summarize_metrics(metrics):
    """ref:lib/tester.py:322-334: '*mse' -> the root of the mean under '*rmse'; 'err*' -> '_mean' and '_rmse'; the rest a mean."""
    summarized = {}
    for k in metrics:
        if k.endswith("mse"):
            summarized[k[:-3] + "rmse"] = np.sqrt(np.mean(metrics[k]))
        elif k.startswith("err"):
            summarized[k + "_mean"] = np.mean(metrics[k])
            summarized[k + "_rmse"] = np.sqrt(np.mean(metrics[k] ** 2))
        else:
            summarized[k] = np.mean(metrics[k])
    return summarized


def print_metrics(summary, title="Metrics", out=print):
    """The lines of the reference's print_metrics (ref:lib/tester.py:300-320), handed to `out` one by one."""
    out(title + ":")
    out("=" * (len(title) + 1))
    out("DeepCP metrics:{:.4f}(rot-rmse) | {:.4f}(rot-mae) | {:.4g}(trans-rmse) | {:.4g}(trans-mae)".format(
        summary["r_rmse"], summary["r_mae"], summary["t_rmse"], summary["t_mae"]))
    out("Rotation error {:.4f}(deg, mean) | {:.4f}(deg, rmse)".format(summary["err_r_deg_mean"], summary["err_r_deg_rmse"]))
    out("Translation error {:.4g}(mean) | {:.4g}(rmse)".format(summary["err_t_mean"], summary["err_t_rmse"]))
    out("Chamfer error: {:.7f}(mean-sq)".format(summary["chamfer_dist"]))
