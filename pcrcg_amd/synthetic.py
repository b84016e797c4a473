"""Synthetic point-cloud recipes shared by tests, smoke() and bench.py.

All generators use ``np.random.RandomState(seed)`` and return float32 arrays.  The ``shell`` recipe
reproduces the neighbourhood statistics of a real 3DMatch fragment pair (points on the faces of a
cube, i.e. 2-D surfaces embedded in 3-D, with a little jitter).
"""
import numpy as np

# name -> (points per cloud, cube side [m], jitter [m])
RECIPES = {
    "C1": (5000, 0.75, 0.02),       # BASELINE.json configs[0]
    "S30k": (30000, 1.3, 0.02),     # BASELINE.json configs[1], "3DMatch-shaped"
    "mini": (1500, 0.45, 0.02),     # small parity case
    "T8k": (8000, 0.9, 0.02),       # tie-rich case: coordinates snapped to a 1/128 m lattice (see pair())
    "T30k": (30000, 1.3, 0.02),     # S30k snapped to a 1/256 m lattice: the bench's "voxelised scan" workload
}
LATTICE = {"T8k": 128.0, "T30k": 256.0}

# neighbourhood limits measured on the recipes with the reference's calibrate_neighbors formula
# (ref:datasets/dataloader.py:402-434); see scripts/make_golden_frontend.py
LIMITS = {
    "C1": [24, 37, 45, 48],
    "S30k": [43, 42, 47, 43],
    "K120k": [62, 58, 60, 60],
    "U30k": [29, 65, 75, 63],      # scripts/calib_u30k.py (pcrcg_amd.pyramid.calibrate_neighbors on the GPU)
}


def shell(rng, n, side, jitter):
    """n points on the six faces of a ``side``-cube plus uniform jitter."""
    face = rng.randint(0, 6, n)
    uv = rng.rand(n, 2).astype(np.float64) * side
    p = np.empty((n, 3), np.float64)
    axis = face // 2                       # the axis normal to the face
    level = (face % 2).astype(np.float64) * side
    for a in range(3):
        sel = axis == a
        o = [d for d in range(3) if d != a]
        p[sel, a] = level[sel]
        p[sel, o[0]] = uv[sel, 0]
        p[sel, o[1]] = uv[sel, 1]
    p += (rng.rand(n, 3) - 0.5) * jitter
    return p.astype(np.float32)


def pair(recipe="S30k", seed=0):
    """(src, tgt) float32 [n,3] clouds; src then tgt drawn from the same stream."""
    n, side, jitter = RECIPES[recipe]
    rng = np.random.RandomState(seed)
    src = shell(rng, n, side, jitter)
    tgt = shell(rng, n, side, jitter)
    if recipe in LATTICE:
        # Real scans (voxelised depth maps) are full of EXACTLY equal point distances and a few duplicate points;
        # uniform random floats have none.  Snapping to a lattice reproduces that: 13 705 of the 16 000 level-0
        # rows of T8k hold a tie group, 517 points are duplicates.
        q = np.float32(LATTICE[recipe])
        src = (np.round(src * q) / q).astype(np.float32)
        tgt = (np.round(tgt * q) / q).astype(np.float32)
    return src, tgt


def uniform_pair(n=30000, side=1.07, seed=0):
    """U30k: uniform-random points in a cube (the north_star's wording; SURVEY.md 8d "uniform-volume
    alternative"): denser neighbourhoods than a surface scan and an 8x decay per level."""
    rng = np.random.RandomState(seed)
    return (rng.rand(n, 3) * side).astype(np.float32), (rng.rand(n, 3) * side).astype(np.float32)


def slab_pair(n=120000, seed=0, extent=104.0, height=0.6):
    """K120k: KITTI-shaped outdoor slab (BASELINE.json configs[4])."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        p = rng.rand(n, 3)
        p[:, :2] *= extent
        p[:, 2] *= height
        out.append(p.astype(np.float32))
    return out[0], out[1]


def lomatch_pair(recipe="S30k", seed=0, overlap=0.2):
    """3DLoMatch-shaped pair (BASELINE.json configs[2]): tgt = R*(subset of src) + t plus fresh
    points so that roughly ``overlap`` of the points coincide.  Returns src, tgt, rot, trans."""
    n, side, jitter = RECIPES[recipe]
    rng = np.random.RandomState(seed)
    src = shell(rng, n, side, jitter)
    k = int(n * overlap)
    keep = rng.permutation(n)[:k]
    fresh = shell(rng, n - k, side, jitter) + np.float32(side * 0.8)
    ang = rng.rand(3) * 2 * np.pi
    cz, sz, cy, sy, cx, sx = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    rot = Rz @ Ry @ Rx
    trans = rng.rand(3, 1) - 0.5
    tgt_src = np.concatenate([src[keep], fresh], 0).astype(np.float64)
    tgt = (rot @ tgt_src.T + trans).T.astype(np.float32)
    return src, tgt, rot.astype(np.float32), trans.astype(np.float32)


def image_inputs(n_src, n_tgt, seed=0, img_num=2, h=120, w=160, frac=0.45, channels=128):
    """Synthetic stand-ins for what PCR-CG's 2-D branch hands to KPFCNN.forward (ref:models/architectures.py:195-514,
    ref:datasets/indoor.py:192-829): per cloud and image a [channels, h, w] feature map (the ResUNet's output shape for the
    3DMatch frames: 128 x 120 x 160), the projected points' pixel coordinates `inds2d` [k, 2] (column, row) and point
    indices `inds3d` [k] -- a random `frac` of the cloud per image, overlapping between images, so the write order matters
    -- and, for img_num < 3, a [w, h] valid mask.  Keys as in the reference's batch dict, with the maps under
    '{side}{i}_feature2d' (what pcrcg_amd.KPFCNN takes in place of a backbone).  numpy arrays, seeded: the same inputs in the
    fixture generator (scripts/make_golden_image_s30k.py), the tests and bench.py."""
    rng = np.random.RandomState(1000 + seed)
    out = {}
    for side, n in (("src", n_src), ("tgt", n_tgt)):
        for i in range(1, img_num + 1):
            k = int(n * frac)
            out[f"{side}{i}_feature2d"] = rng.rand(channels, h, w).astype(np.float32)
            out[f"{side}{i}_inds3d"] = rng.permutation(n)[:k].astype(np.int64)
            out[f"{side}{i}_inds2d"] = np.stack([rng.randint(0, w, k), rng.randint(0, h, k)], 1).astype(np.int64)
            if img_num < 3:
                out[f"{side}_valid_map{i}"] = (rng.rand(w, h) > 0.2).astype(np.float32)
    return out


# the 3DMatch intrinsics (fx = fy = 585, cx = 320, cy = 240 at 640 x 480) scaled to the 160 x 120 frames the 2-D branch uses
INTRINSICS_160 = np.array([[146.25, 0.0, 80.0], [0.0, 146.25, 60.0], [0.0, 0.0, 1.0]], np.float32)


def render_depth(points, world2camera, intrinsics=INTRINSICS_160, h=120, w=160, rng=None, noise=0.04, drop=0.05):
    """A z-buffered depth map [h, w] f32 of `points` seen through world2camera (4x4) and intrinsics (3x3): the nearest
    point per pixel, 0 where none lands (a missing depth pixel), then Gaussian noise of `noise` m on the filled pixels and
    a `drop` share of them zeroed -- so that the depth test of a projection rejects some of the points."""
    p = points.astype(np.float64) @ world2camera[:3, :3].astype(np.float64).T + world2camera[:3, 3].astype(np.float64)
    z = p[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = intrinsics[0, 0] * p[:, 0] / z + intrinsics[0, 2]
        v = intrinsics[1, 1] * p[:, 1] / z + intrinsics[1, 2]
    ok = (z > 0.05) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
    flat = v[ok].astype(np.int64) * w + u[ok].astype(np.int64)
    depth = np.full(h * w, np.inf)
    np.minimum.at(depth, flat, z[ok])
    depth[np.isinf(depth)] = 0.0
    if rng is not None:
        filled = depth > 0
        depth[filled] += rng.normal(0.0, noise, int(filled.sum()))
        depth[filled & (rng.rand(h * w) < drop)] = 0.0
    return depth.reshape(h, w).astype(np.float32)


def _pose(rng, angle=0.12, shift=0.15):
    """A camera pose (4x4 f64): a rotation of up to `angle` rad about a random axis and a shift of up to `shift` m."""
    ax = rng.randn(3)
    ax /= np.linalg.norm(ax)
    a = (rng.rand() * 2 - 1) * angle
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    pose = np.eye(4)
    pose[:3, :3] = np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k)
    pose[:3, 3] = (rng.rand(3) * 2 - 1) * shift
    return pose


def second_world2camera(pose1, pose2, world2camera1):
    """Image 2's world2camera as the reference composes it (ref:datasets/indoor.py:587-592): pose2^-1 . pose1 .
    world2camera1, the inverse in float64 numpy, the products in float32 torch."""
    import torch
    return torch.mm(torch.from_numpy(np.linalg.inv(pose2)).float(),
                    torch.mm(torch.from_numpy(pose1).float(), torch.from_numpy(world2camera1).float())).numpy()


def superglue_like(rng, n0=400, n1=450, unmatched=0.3, h=120, w=160):
    """SuperGlue-shaped output of one image pair: keypoints0 [n0, 2], keypoints1 [n1, 2] f32 (x, y), matches [n0] i64
    (-1: unmatched), match_confidence [n0] f32."""
    kp0 = (rng.rand(n0, 2) * [w, h]).astype(np.float32)
    kp1 = (rng.rand(n1, 2) * [w, h]).astype(np.float32)
    m = min(n0, n1)
    matches = np.full(n0, -1, np.int64)
    matches[rng.permutation(n0)[:m]] = rng.permutation(n1)[:m]     # one-to-one, as SuperGlue's mutual matches are
    matches[rng.rand(n0) < unmatched] = -1
    return dict(keypoints0=kp0, keypoints1=kp1, matches=matches, confidence=rng.rand(n0).astype(np.float32))


def frame_inputs(src, tgt, seed=0, img_num=2, h=120, w=160, channels=128):
    """Raw frames for the device projection (pcrcg_inject_frames): per cloud and image a random [channels, h, w] feature
    map, a depth map z-buffer-rendered from the cloud (render_depth: noise and dropped pixels, so the depth test rejects a
    share of the points), world2camera [4, 4] and the 3DMatch intrinsics at 160 x 120 [3, 3].  Image 1 looks at the cloud
    from in front of its centre; images 2 and 3 from a pose offset, their world2camera composed the way the reference
    composes it (second_world2camera).  For img_num < 3, SuperGlue-like matches per image under 'sg{i}_{keypoints0,
    keypoints1,matches,confidence}' (superglue_valid_maps paints the valid maps from them).  Keys as in the reference's
    batch dict ('{side}{i}_depth', '{side}{i}_world2camera', '{side}{i}_intrinsics'; maps under '{side}{i}_feature2d').
    numpy arrays, seeded."""
    rng = np.random.RandomState(2000 + seed)
    out = {}
    for side, pts in (("src", src), ("tgt", tgt)):
        w2c1 = np.eye(4, dtype=np.float32)
        lo, hi = pts.min(0), pts.max(0)
        w2c1[:3, 3] = [-(lo[0] + hi[0]) / 2, -(lo[1] + hi[1]) / 2, 0.8 - lo[2] + 0.5 * (hi[0] - lo[0])]
        pose1 = np.eye(4)
        for i in range(1, img_num + 1):
            w2c = w2c1 if i == 1 else second_world2camera(pose1, _pose(rng), w2c1)
            out[f"{side}{i}_feature2d"] = rng.rand(channels, h, w).astype(np.float32)
            out[f"{side}{i}_depth"] = render_depth(pts, w2c, h=h, w=w, rng=rng)
            out[f"{side}{i}_world2camera"] = w2c.astype(np.float32)
            out[f"{side}{i}_intrinsics"] = INTRINSICS_160.copy()
    if img_num < 3:
        for i in range(1, img_num + 1):
            for k, v in superglue_like(rng, h=h, w=w).items():
                out[f"sg{i}_{k}"] = v
    return out


def modelnet_pairs(B, seed, n=1024, keep=0.7, n_raw=2048):
    """B ModelNet-shaped pairs (ref:datasets/modelnet.py through its transforms: a clean cloud, two resampled partial
    views of it, the source view moved away by a rigid transform) -> list of dicts of float32 arrays:
      points_raw [n_raw, 3]  the clean cloud: a torus with a wavy tube in the unit cube, no symmetry to speak of (the
                             surface of scripts/make_golden_modelnet.py::modelnet_pair), in the reference frame;
      points_ref [round(n keep), 3]  n of its points, jittered, cropped by a random half-space to `keep`;
      points_src [round(n keep), 3]  the same with another jitter and half-space, moved by transform_gt^-1;
      transform_gt [3, 4]    source -> reference: a rotation of up to 45 degrees about a random axis and a translation
                             of up to 0.5 per axis (the range of the reference's RandomTransformSE3_euler).
    So transform_gt * points_src lies on points_raw, as compute_metrics assumes."""
    out = []
    for b in range(B):
        rng = np.random.RandomState([seed, b])
        u, v = rng.rand(n_raw) * 2 * np.pi, rng.rand(n_raw) * 2 * np.pi
        r_major, r_minor = 0.6, 0.25 + 0.08 * np.sin(3 * u)
        raw = np.stack([(r_major + r_minor * np.cos(v)) * np.cos(u), (r_major + r_minor * np.cos(v)) * np.sin(u),
                        r_minor * np.sin(v)], 1)
        views = []
        for _ in range(2):
            p = raw[rng.permutation(n_raw)[:n]] if n <= n_raw else raw[rng.randint(0, n_raw, n)]
            p = p + np.clip(rng.randn(n, 3) * 0.01, -0.05, 0.05)
            d = rng.randn(3)
            d /= np.linalg.norm(d)
            views.append(p[np.argsort(p @ d)[:int(round(n * keep))]])
        pose = _pose(rng, angle=np.pi / 4, shift=0.5)
        rot, t = pose[:3, :3], pose[:3, 3]
        src = (views[0] - t) @ rot                      # rot^T (p - t), row by row
        out.append({"points_src": src.astype(np.float32), "points_ref": views[1].astype(np.float32),
                    "points_raw": raw.astype(np.float32), "transform_gt": pose[:3].astype(np.float32)})
    return out


def modelnet_clouds(S, seed, n_raw=2048):
    """S ModelNet-shaped raw clouds with normals, what ref:datasets/modelnet.py _read_h5_files returns as `data`
    ([S, n_raw, 6] float32: xyz and unit normals): the wavy torus of modelnet_pairs with its analytic normals (the
    normalised cross product of the surface's two partial derivatives).  Input of modelnet_prep.prepare_pairs."""
    out = np.empty((S, n_raw, 6), dtype=np.float32)
    for b in range(S):
        rng = np.random.RandomState([seed, b])
        u, v = rng.rand(n_raw) * 2 * np.pi, rng.rand(n_raw) * 2 * np.pi
        r_major, r_minor, d_minor = 0.6, 0.25 + 0.08 * np.sin(3 * u), 0.24 * np.cos(3 * u)
        w = r_major + r_minor * np.cos(v)
        p = np.stack([w * np.cos(u), w * np.sin(u), r_minor * np.sin(v)], 1)
        du = np.stack([d_minor * np.cos(v) * np.cos(u) - w * np.sin(u), d_minor * np.cos(v) * np.sin(u) + w * np.cos(u),
                       d_minor * np.sin(v)], 1)
        dv = np.stack([-r_minor * np.sin(v) * np.cos(u), -r_minor * np.sin(v) * np.sin(u), r_minor * np.cos(v)], 1)
        nrm = np.cross(du, dv)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        out[b] = np.concatenate([p, nrm], 1)
    return out
