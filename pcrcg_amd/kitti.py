"""Preparing KITTI pairs on the device: the body of ref:datasets/kitti.py KITTIDataset.__getitem__ after the two scans
and the odometry pose are read (:105-182), without open3d or scipy.

  * `voxel_down_sample_batch` -- open3d's `pcd.voxel_down_sample(voxel_size)` for many clouds in ONE library call
                                 (pcrcg_voxel_down_sample_batch; include/pcrcg.h "Voxel down-sampling", DESIGN.md section
                                 14); `voxel_down_sample` is a batch of one.  The same primitive makes the 2.5 cm clouds
                                 of ref:datasets/indoor.py from raw 3DMatch fragments.
  * `prepare_pairs`           -- :105-151 for B pairs: the refined pose M2 (cached, or registration.refine_ground_truth),
                                 all 2 B scans down-sampled in one call, ground-truth correspondences per pair, and one
                                 dict per pair with the keys pyramid.collate_fn_descriptor reads; `prepare_pair` is one pair.
  * `augment`                 -- :156-179: the draws on the host in the reference's order and shapes, applied on the device.

Row order: open3d emits the down-sampled rows in its hash map's iteration order; here they come in ascending index of each
voxel's first input point (no bit parity with open3d is claimed).  The reference's consumers take the clouds as they come,
so every index in `correspondences` refers to the rows this module returns.
"""
import numpy as np
import torch

from . import _lib, ragged
from .config import as_config
from .correspondences import get_correspondences

_MAX_BATCH = 65535          # pcrcg_voxel_down_sample_batch: B
_MAX_ROWS = 1 << 30         # ... and n_total


def _device(clouds):
    return ragged.device(clouds, "kitti")


def _rows(x, who, b):
    shape = ragged.shape_of(x)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{who}: cloud {b} must be an [N, 3] array, got shape {shape}")
    return shape[0]


def voxel_down_sample_batch(clouds, voxel_size, *, with_index=False):
    """open3d's voxel_down_sample for a list of [N_b,3] clouds (numpy, CPU or HIP tensors; rounded to fp32, what a KITTI
    .bin holds) -> a list of [K_b,3] float64 device tensors, rows in ascending index of each voxel's first input point.
    with_index=True: -> (points, first, count), two more lists of [K_b] int32 device tensors: the index of the first input
    point of every row's voxel, and how many points the row averaged.

    One library call and one read-back (the B output lengths).  A cloud with a non-finite coordinate, or one whose extent
    over voxel_size reaches 2^21 on an axis (open3d: "voxel_size is too small"), raises ValueError naming the cloud."""
    clouds = list(clouds)
    B = len(clouds)
    if B == 0:
        raise ValueError("voxel_down_sample_batch: no clouds")
    if B > _MAX_BATCH:
        raise ValueError(f"voxel_down_sample_batch: {B} clouds in one call, at most {_MAX_BATCH}")
    vs = float(voxel_size)
    if not (0.0 < vs < float("inf")):
        raise ValueError(f"voxel_down_sample_batch: voxel_size must be positive and finite, got {voxel_size!r}")
    ns = [_rows(x, "voxel_down_sample_batch", b) for b, x in enumerate(clouds)]
    n_total = sum(ns)
    if n_total > _MAX_ROWS:
        raise ValueError(f"voxel_down_sample_batch: {n_total} rows in one call, at most {_MAX_ROWS}")
    dev = _device(clouds)
    L = _lib.lib()
    pts = (ragged.upload(clouds, dev, torch.float32, 3, "clouds") if n_total
           else torch.zeros((1, 3), dtype=torch.float32, device=dev))    # all clouds empty: a placeholder row, not read
    off, = ragged.offsets(dev, ns)
    cap = max(n_total, 1)
    out = torch.empty((cap, 3), dtype=torch.float64, device=dev)
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    first = torch.empty(cap, dtype=torch.int32, device=dev) if with_index else None
    count = torch.empty(cap, dtype=torch.int32, device=dev) if with_index else None
    wsb = L.pcrcg_voxel_down_sample_ws_bytes(B, n_total)
    if wsb == 0:
        raise ValueError("voxel_down_sample_batch: sizes out of range for the workspace")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.pcrcg_voxel_down_sample_batch(pts.data_ptr(), off.data_ptr(), n_total, B, vs, out.data_ptr(), out_len.data_ptr(),
                                               first.data_ptr() if with_index else None,
                                               count.data_ptr() if with_index else None, ws.data_ptr(), wsb,
                                               torch.cuda.current_stream(dev).cuda_stream), "pcrcg_voxel_down_sample_batch")
    lens = out_len.cpu().tolist()                     # the ONE read-back
    for b, k in enumerate(lens):
        if k < 0:
            raise ValueError(f"voxel_down_sample_batch: cloud {b} was rejected: it has a non-finite coordinate, or voxel_size "
                             f"{vs} is too small for its extent (an index would reach 2^21)")
    points = list(out[:sum(lens)].split(lens))
    if not with_index:
        return points
    return points, list(first[:sum(lens)].split(lens)), list(count[:sum(lens)].split(lens))


def voxel_down_sample(cloud, voxel_size):
    """One cloud -> [K,3] float64 device tensor: voxel_down_sample_batch with a batch of one."""
    return voxel_down_sample_batch([cloud], voxel_size)[0]


def euler_zyx_matrix(angles):
    """scipy's Rotation.from_euler('zyx', angles).as_matrix() in float64 numpy: extrinsic rotations about z, then y, then x,
    i.e. Rx(angles[2]) @ Ry(angles[1]) @ Rz(angles[0])."""
    az, ay, ax = (float(a) for a in angles)
    cz, sz, cy, sy, cx, sx = np.cos(az), np.sin(az), np.cos(ay), np.sin(ay), np.cos(ax), np.sin(ax)
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    return Rx @ Ry @ Rz


def augment_draws(n_src, n_tgt, config, rng):
    """The random numbers of ref:datasets/kitti.py:158-176, drawn on the host in the reference's call order and shapes.
    rng = (numpy.random.RandomState, random.Random): the reference draws from numpy's global state everywhere except the
    scale, which comes from the `random` module.  -> dict of float64 numpy values."""
    np_rng, py_rng = rng
    d = {}
    d["noise_src"] = (np_rng.rand(n_src, 3) - 0.5) * config.augment_noise                     # :158
    d["noise_tgt"] = (np_rng.rand(n_tgt, 3) - 0.5) * config.augment_noise                     # :159
    d["euler"] = np_rng.rand(3) * np.pi * 2                                                    # :162
    d["rot"] = euler_zyx_matrix(d["euler"])                                                    # :163
    d["rotate_src"] = bool(np_rng.rand(1)[0] > 0.5)                                            # :164
    d["scale"] = config.augment_scale_min + (config.augment_scale_max - config.augment_scale_min) * py_rng.random()   # :170
    d["shift_src"] = np_rng.uniform(-config.augment_shift_range, config.augment_shift_range, 3)   # :175
    d["shift_tgt"] = np_rng.uniform(-config.augment_shift_range, config.augment_shift_range, 3)   # :176
    return d


def _rotate(pts, rot):
    """np.dot(rot, pts.T).T row by row, the three products added left to right."""
    x, y, z = pts[:, 0:1], pts[:, 1:2], pts[:, 2:3]
    return (x * rot[:, 0] + y * rot[:, 1]) + z * rot[:, 2]


def augment(src, tgt, config, rng):
    """ref:datasets/kitti.py:156-179 -> (src_input, tgt_input), float64 device tensors: noise, then ONE rotation applied to
    the source or to the target, then the scale, then the two shifts.  src, tgt: [N,3] / [M,3] clouds (device tensors stay
    where they are).  rng = (numpy.random.RandomState, random.Random), consumed in the reference's call order and shapes
    (augment_draws): a caller who seeds both as the reference's process seeds numpy and `random` gets the reference's
    draws.  The draws happen on the host; the arithmetic is float64 torch on the device.  config: augment_noise,
    augment_scale_min, augment_scale_max, augment_shift_range (ref:configs/train/kitti.yaml)."""
    config = as_config(config)
    dev = _device([src, tgt])
    s = (src if isinstance(src, torch.Tensor) else torch.as_tensor(np.asarray(src))).to(device=dev, dtype=torch.float64)
    t = (tgt if isinstance(tgt, torch.Tensor) else torch.as_tensor(np.asarray(tgt))).to(device=dev, dtype=torch.float64)
    _rows(s, "augment", 0), _rows(t, "augment", 1)
    d = augment_draws(s.shape[0], t.shape[0], config, rng)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    s = s + up(d["noise_src"])
    t = t + up(d["noise_tgt"])
    if d["rotate_src"]:
        s = _rotate(s, up(d["rot"]))
    else:
        t = _rotate(t, up(d["rot"]))
    s = s * d["scale"]
    t = t * d["scale"]
    return s + up(d["shift_src"]), t + up(d["shift_tgt"])


_augment = augment      # (prepare_pairs has a keyword of that name)


def prepare_pairs(scans0, scans1, poses, config, *, refined=None, augment=None):
    """ref:datasets/kitti.py:105-182 for B pairs -> a list of B dicts, what pyramid.collate_fn_descriptor takes.

    scans0[b], scans1[b]: the raw scans' [N,3] xyz (numpy, CPU or HIP tensors).  poses[b]: the [4,4] odometry pose M of :111.
    refined: None, or a list whose entry b is the cached refined pose M2 of pair b (the reference's icp/*.npy) or None;
    where it is missing, registration.refine_ground_truth(scans0[b], scans1[b], M) computes it.  All 2 B scans are
    down-sampled in ONE voxel_down_sample_batch call at config.first_subsampling_dl; get_correspondences then runs per pair
    under M2 with radius config.overlap_radius.  augment: None, or rng = (numpy.random.RandomState, random.Random): the
    network's clouds are then `augment`'s, pair by pair in order.

    Every dict holds src_pcd, tgt_pcd (fp32 device tensors: the network's input), src_feats, tgt_feats (ones, [N,1] fp32),
    rot [3,3] and trans [3,1] (fp32 numpy, M2's), correspondences ([K,2] int64 device), src_pcd_raw, tgt_pcd_raw (the
    down-sampled clouds before augmentation in float64: the reference tuple's src_pcd, tgt_pcd), sample=None and
    n_correspondences.  The train split's redraw rule (:144, fewer than config.max_points correspondences: draw another
    pair) stays with the caller, which has n_correspondences to apply it.

    The reference searches the correspondences among the float64 down-sampled clouds; this searches what the network is
    fed, the same clouds rounded to fp32, so a pair within fp32 rounding of the radius may differ."""
    config = as_config(config)
    B = len(scans0)
    if B == 0:
        raise ValueError("prepare_pairs: no pairs")
    if len(scans1) != B or len(poses) != B:
        raise ValueError(f"prepare_pairs: list lengths differ ({B}, {len(scans1)}, {len(poses)})")
    if refined is not None and len(refined) != B:
        raise ValueError(f"prepare_pairs: refined has {len(refined)} entries for {B} pairs")
    for b in range(B):
        _rows(scans0[b], "prepare_pairs: scans0", b)
        _rows(scans1[b], "prepare_pairs: scans1", b)

    def pose(M, what, b):
        M = np.asarray(M.cpu() if isinstance(M, torch.Tensor) else M, dtype=np.float64)
        if M.shape != (4, 4):
            raise ValueError(f"prepare_pairs: pair {b}: {what} must be a [4, 4] transform, got shape {M.shape}")
        return M

    Ms = [pose(M, "the pose", b) for b, M in enumerate(poses)]
    M2s = [pose(refined[b], "the refined pose", b) if refined is not None and refined[b] is not None else None for b in range(B)]
    from . import registration
    for b in range(B):
        if M2s[b] is None:
            M2s[b] = registration.refine_ground_truth(scans0[b], scans1[b], Ms[b])
    down = voxel_down_sample_batch(list(scans0) + list(scans1), config.first_subsampling_dl)
    items = []
    for b in range(B):
        src64, tgt64 = down[b], down[B + b]
        src, tgt = src64.float(), tgt64.float()
        corr = get_correspondences(src, tgt, M2s[b], config.overlap_radius)
        src_in, tgt_in = src, tgt
        if augment is not None:
            src_in, tgt_in = (x.float() for x in _augment(src64, tgt64, config, augment))
        dev = src.device
        items.append({
            "src_pcd": src_in, "tgt_pcd": tgt_in,
            "src_feats": torch.ones((src.shape[0], 1), dtype=torch.float32, device=dev),
            "tgt_feats": torch.ones((tgt.shape[0], 1), dtype=torch.float32, device=dev),
            "rot": M2s[b][:3, :3].astype(np.float32), "trans": M2s[b][:3, 3][:, None].astype(np.float32),
            "correspondences": corr, "src_pcd_raw": src64, "tgt_pcd_raw": tgt64, "sample": None,
            "n_correspondences": int(corr.shape[0]),
        })
    return items


def prepare_pair(scan0, scan1, pose, config, *, refined=None, augment=None):
    """One pair -> its dict: prepare_pairs with a batch of one."""
    return prepare_pairs([scan0], [scan1], [pose], config, refined=None if refined is None else [refined], augment=augment)[0]
