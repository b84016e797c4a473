"""numpy restatements of PCR-CG's projection (ref:projection.py Projection.projection) and of the loader's SuperGlue
valid-map painting (ref:datasets/indoor.py:284-299), for the CPU tests of pcrcg_amd.projection.

The projection rounds like the reference's two CPU torch.mm calls: per output value the k-ordered fused chain
fma(m3, 1, fma(m2, p2, fma(m1, p1, m0 * p0))).  numpy has no fma, so `fmaf` below is an exact one: the product of two
float32 values is exact in float64, the sum is formed with TwoSum and rounded to odd in float64, and rounding that to
float32 is then the correctly rounded a * b + c (53 >= 2 * 24 + 2 bits)."""
import numpy as np

F32, F64 = np.float32, np.float64


def fmaf(a, b, c):
    """Correctly rounded float32 a * b + c, elementwise (a, b, c float32 arrays)."""
    p = a.astype(F64) * b.astype(F64)                   # exact
    c = c.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                  # p + c = s + err exactly (finite values)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = s.copy()
        s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))    # round to odd
        return s.astype(F32)


def mm_rows(m, p):
    """torch.mm(m, [p.T; 1]).T[:, :3] as the reference's CPU GEMM rounds it: m [4, 4] f32, p [n, 3] f32."""
    m = np.asarray(m, F32)
    out = np.empty((p.shape[0], 3), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            a = (F32(m[r, 0]) * p[:, 0]).astype(F32)
            a = fmaf(np.full_like(a, m[r, 1]), p[:, 1], a)
            a = fmaf(np.full_like(a, m[r, 2]), p[:, 2], a)
            out[:, r] = fmaf(np.full_like(a, m[r, 3]), np.ones_like(a), a)
    return out


def as4(m):
    m = np.asarray(m, F32)
    if m.shape == (3, 3):
        e = np.eye(4, dtype=F32)
        e[:3, :3] = m
        m = e
    return m


def project(points, depth, world2camera, intrinsics, thresh=0.1):
    """-> (inds2d [k, 2] i64 (column, row), inds3d [k] i64) as Projection.projection returns them."""
    depth = np.asarray(depth, F32).reshape(depth.shape[-2:])
    h, w = depth.shape
    img = mm_rows(as4(intrinsics), mm_rows(as4(world2camera), np.asarray(points, F32)))
    z = img[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        qx, qy = img[:, 0] / z, img[:, 1] / z
        keep = (qx > -1) & (qx < w) & (qy > -1) & (qy < h)     # .long() truncates toward zero; NaN / inf are masked
    px = np.where(keep, qx, 0).astype(np.int64)
    py = np.where(keep, qy, 0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        keep &= np.abs(z - depth[py, px]) < F32(thresh)
    idx = np.nonzero(keep)[0]
    return np.stack([px[idx], py[idx]], 1), idx.astype(np.int64)


def paint_valid_maps(keypoints0, keypoints1, matches, confidence, window=5, size=(160, 120)):
    """The loader's valid maps, with numpy's own slice assignment (so numpy's slice rules are the ones used).  The
    keypoint arithmetic is exact (float64), as in the reference's numpy float64 scalar arithmetic."""
    src, tgt = np.zeros(size, F32), np.zeros(size, F32)
    valid = matches > -1
    k0 = keypoints0[valid].astype(F64)
    k1 = keypoints1[matches[valid]].astype(F64)
    conf = confidence[valid]
    for i in range(len(k0)):
        for m, k in ((src, k0[i]), (tgt, k1[i])):
            m[int(k[0] - window):int(k[0] + window), int(k[1] - window):int(k[1] + window)] = conf[i]
    return src, tgt


def load_fixture(golden_dir):
    """tests/golden/projection.npz (scripts/make_golden_projection.py) as torch tensors:
    {"projection": [{name, points, depth, world2camera, intrinsics, inds2d, inds3d}], "valid_maps": [{keypoints0,
    keypoints1, matches, confidence, src_valid, tgt_valid}], "window"}."""
    import os
    import torch
    z = np.load(os.path.join(golden_dir, "projection.npz"))
    K = torch.from_numpy(z["intrinsics"])
    cases = []
    for j in range(int(z["n_cases"])):
        pts = z[f"cloud/{z[f'{j}/cloud']}"]
        keep = np.unpackbits(z[f"{j}/keep"], count=len(pts)).astype(bool)
        cases.append(dict(name=str(z[f"{j}/name"]), points=torch.from_numpy(pts),
                          depth=torch.from_numpy(z[f"{j}/depth"].astype(F32)),
                          world2camera=torch.from_numpy(z[f"{j}/world2camera"]), intrinsics=K,
                          inds2d=torch.from_numpy(z[f"{j}/inds2d"].astype(np.int64)),
                          inds3d=torch.from_numpy(np.nonzero(keep)[0].astype(np.int64))))
    valid = []
    j = 0
    while f"valid{j}/matches" in z:
        v = {k: z[f"valid{j}/{k}"] for k in ("keypoints0", "keypoints1", "matches", "confidence", "src_idx", "tgt_idx")}
        conf = np.concatenate([[F32(0)], v["confidence"][v["matches"] > -1]]).astype(F32)
        v["src_valid"], v["tgt_valid"] = conf[v.pop("src_idx")], conf[v.pop("tgt_idx")]
        valid.append({k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in v.items()})
        j += 1
    return dict(projection=cases, valid_maps=valid, window=int(z["window"]))


def load_edges(golden_dir):
    """tests/golden/projection_edges.npz (scripts/make_golden_projection_edges.py): the reference's own output at the
    projection's decision boundaries, as numpy arrays: [{name, points, depth ([H, W] or [1, H, W]), world2camera,
    intrinsics (3x3 or 4x4), thresh, inds2d, inds3d}]."""
    import os
    z = np.load(os.path.join(golden_dir, "projection_edges.npz"))
    cases = []
    for j in range(int(z["n_cases"])):
        pts = z[f"{j}/points"]
        keep = np.unpackbits(z[f"{j}/keep"], count=len(pts)).astype(bool)
        cases.append(dict(name=str(z[f"{j}/name"]), points=pts, depth=z[f"{j}/depth"], world2camera=z[f"{j}/world2camera"],
                          intrinsics=z[f"{j}/intrinsics"], thresh=float(z[f"{j}/thresh"]),
                          inds2d=z[f"{j}/inds2d"].astype(np.int64).reshape(-1, 2), inds3d=np.nonzero(keep)[0].astype(np.int64)))
    return cases


def inject_frames_ref(points, len_src, frames, c, ldx):
    """include/pcrcg.h's rule for pcrcg_inject_frames, from project() alone: x [n, ldx] f32 = ones in columns 0..c and
    zeros after; then per frame in write order, on the rows of its cloud that project() keeps,
    x[rows, :c] = fmap[:, py, px].T * valid[px, py].  points [n, 3] (len_src source rows first); frames: dicts of numpy
    arrays fmap [c, h, w], depth [h, w], world2camera, intrinsics, target, optionally valid [w, h] and thresh.
    -> (x, winner [n] = the index of the frame each row took, -1: none)."""
    points = np.asarray(points, F32)
    n = len(points)
    x = np.zeros((n, ldx), F32)
    x[:, :c + 1] = 1
    winner = np.full(n, -1, np.int64)
    for j, fr in enumerate(frames):
        lo, hi = (len_src, n) if fr.get("target") else (0, len_src)
        i2, i3 = project(points[lo:hi], fr["depth"], fr["world2camera"], fr["intrinsics"], fr.get("thresh", 0.1))
        feats = np.asarray(fr["fmap"], F32)[:, i2[:, 1], i2[:, 0]].T
        if fr.get("valid") is not None:
            feats = feats * np.asarray(fr["valid"], F32)[i2[:, 0], i2[:, 1]][:, None]
        x[lo + i3, :c] = feats
        winner[lo + i3] = j
    return x, winner
