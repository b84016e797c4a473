"""tests/golden/projection_edges.npz: the UNMODIFIED reference's Projection.projection (ref:projection.py, build container
only) at the decision boundaries of the projection, on inputs whose arithmetic is exact in float32.

Every case uses an axis-permutation (or identity) rotation, a translation on the 1/64 lattice and power-of-two focal
lengths, and its points are built backwards from the image-space values they are meant to hit: quotients (qx, qy) and
depth z.  Where z is a power of two the whole chain -- both matrix products and the perspective division -- is exact,
so neither the fused rounding nor the GEMM's summation order can move a point off its boundary; main() asserts that
(the float32 chain rounded after every operation equals the float64 one, and the quotients are the intended ones).
The few classes that need a z one ulp off a lattice value sit on the optical axis (quotient 0 / z = 0 exactly).

Classes (each on either side of its boundary): quotient -1, just above -1, in (-1, 0), 0; quotient w / h and the
largest float below; z = 0 with a positive, negative and zero numerator; z < 0 with a depth that accepts it; NaN and
+-inf coordinates; |z - depth| = thresh, one ulp below, thresh = 0; depth NaN / inf / 0 at the hit pixel; a 37 x 53
frame under a permuted, translated pose; a 1 x 1 frame; 3x3 and 4x4 intrinsics; one [1, H, W] depth map.

Stored per case: points, depth (float32), world2camera, intrinsics, thresh, and the reference's result as a keep mask
over the points (inds3d ascends) with inds2d in bytes.  tests/projection_ref.load_edges() rebuilds the tensors.  The
archive is written with fixed member timestamps: a rerun reproduces the file byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

OUT = os.path.join(ref_import.REPO, "tests", "golden", "projection_edges.npz")
F32, F64 = np.float32, np.float64
INF = F32(np.inf)


def below(v):
    return np.nextafter(F32(v), -INF)


def above(v):
    return np.nextafter(F32(v), INF)


def intrinsics(f, cx, cy, four=False):
    K = np.eye(4 if four else 3, dtype=F32)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = cx, cy
    return K


def pose(perm=(0, 1, 2), signs=(1, 1, 1), t=(0, 0, 0)):
    """camera = R world + t with R a signed axis permutation: camera axis r reads world axis perm[r]."""
    m = np.eye(4, dtype=F32)
    m[:3, :3] = 0
    for r in range(3):
        m[r, perm[r]] = signs[r]
    m[:3, 3] = t
    return m


def exact32(v):
    v = np.asarray(v, F64)
    r = v.astype(F32)
    same = (r.astype(F64) == v) | np.isnan(v)
    assert same.all(), v[~same]
    return r


def world_of(cam, w2c):
    """The world points that the (exact) pose maps onto the camera-space points `cam` [n, 3] f64: axis by axis, so a
    non-finite coordinate stays in its own slot."""
    cam = np.asarray(cam, F64)
    world = np.empty_like(cam)
    for r in range(3):
        a = int(np.nonzero(w2c[r, :3])[0][0])
        with np.errstate(invalid="ignore"):
            world[:, a] = (cam[:, r] - F64(w2c[r, 3])) * F64(w2c[r, a])
    return exact32(world)


def cam_of(q, z, K):
    """Camera-space points whose image is quotients q [n, 2] at depth z [n] (f64 in, exact f32 checked by world_of)."""
    q, z = np.asarray(q, F64), np.asarray(z, F64)
    f, cx, cy = F64(K[0, 0]), F64(K[0, 2]), F64(K[1, 2])
    return np.stack([(q[:, 0] - cx) * z / f, (q[:, 1] - cy) * z / f, z], 1)


def border_values(n):
    """Quotients on either side of both ends of an axis of n pixels (f = 1, c = 0, z a power of two: all exact)."""
    return [-2.0, below(-1), -1.0, above(-1), -0.75, -0.5, -2.0 ** -24, -0.0, 0.0, 2.0 ** -20, 0.5, 1.0, n - 1.5, n - 1.0,
            n - 0.5, below(n), float(n), above(n), n + 1.0]


def cross(w, h, xs, ys):
    """xs against the middle row, ys against the middle column, and the pairs of the extremes."""
    mx, my = w // 2 + 0.5, h // 2 + 0.5
    q = [(x, my) for x in xs] + [(mx, y) for y in ys]
    q += [(x, y) for x in xs[1:6] + xs[-6:-1] for y in ys[1:6] + ys[-6:-1]]
    return np.array(q, F64)


def cases():
    out = []

    def add(name, q, z, w, h, K, w2c, depth, thresh=0.125, cam=None, squeeze=False):
        cam = cam_of(q, np.broadcast_to(np.asarray(z, F64), (len(q),)), K) if cam is None else np.asarray(cam, F64)
        depth = np.broadcast_to(np.asarray(depth, F32), (h, w)).copy()
        out.append(dict(name=name, points=world_of(cam, w2c), depth=depth[None] if squeeze else depth, K=K, w2c=w2c,
                        thresh=F32(thresh)))

    # quotient borders through unit intrinsics (q = X / z), z a power of two, the depth map at z
    for z in (1.0, 2.0, 0.5):
        add(f"borders_f1_z{z}", cross(160, 120, border_values(160), border_values(120)), z, 160, 120,
            intrinsics(1, 0, 0), pose(), z, squeeze=z == 2.0)
    # the same borders on the lattice: f = 64, c on the lattice, z = 2 -> half-integer quotients, permuted + translated pose
    half = lambda n: [-1.5, -1.0, -0.5, 0.0, 0.5, n - 1.0, n - 0.5, float(n), n + 0.5]      # noqa: E731
    d = np.full((120, 160), 2.0, F32)
    d[:, 0] = 2.125                                        # column 0: |z - d| = thresh exactly -> rejected
    d[0, 1:] = 2.0 + 7 / 64                                # row 0: inside
    add("borders_f64_perm", cross(160, 120, half(160), half(120)), 2.0, 160, 120, intrinsics(64, 80, 60, four=True),
        pose((2, 0, 1), (1, -1, 1), (0.25, -0.5, 1.0)), d)
    # z = 0 (and -0): the numerators positive, negative and zero on either axis; a depth of 0 would accept any of them
    num = [(x, y) for x in (0.0, 0.5, -0.5, 40.0) for y in (0.0, 0.25, -0.25, 30.0)]
    for K, tag in ((intrinsics(1, 0, 0), "f1"), (intrinsics(64, 80, 60, four=True), "f64")):
        cam = [(x, y, z) for z in (0.0, -0.0) for x, y in num] + [(8.5, 8.5, 1 / 16), (0.0, 0.0, 1 / 16)]
        add(f"z_zero_{tag}", None, None, 160, 120, K, pose(), 0.0, cam=cam)
    # z < 0 with a depth that accepts it: depth 0 within thresh, depth -1 at the pixel; z = -1/8 is exactly thresh away
    q = np.array([(x + 0.5, y + 0.5) for x in (0, 3, 80, 159) for y in (0, 60, 119)], F64)
    for z in (-1 / 64, -1 / 16, -1 / 8, -1.0):
        d = np.zeros((120, 160), F32)
        d[60:, :] = -1.0
        d[119, 159] = 1.0
        add(f"behind_z{z}", q, z, 160, 120, intrinsics(1, 0, 0), pose(), d)
    add("behind_perm", q, -1 / 16, 160, 120, intrinsics(64, 80, 60), pose((1, 2, 0), (-1, 1, 1), (1.0, 0.5, -0.25)), 0.0)
    # non-finite coordinates among ordinary points
    cam = []
    for bad in (np.nan, np.inf, -np.inf):
        for slot in ((0,), (1,), (2,), (0, 1), (0, 2), (0, 1, 2)):
            p = [20.5, 30.5, 1.0]
            for s in slot:
                p[s] = bad
            cam += [p, [20.5, 30.5, 1.0], [0.0, 0.0, 1.0]]
    add("nonfinite", None, None, 160, 120, intrinsics(1, 0, 0), pose(), 1.0, cam=cam)
    add("nonfinite_perm", None, None, 160, 120, intrinsics(1, 0, 0), pose((2, 0, 1), (1, 1, -1)), 1.0, cam=cam)
    # the depth test: |z - d| at thresh, one ulp either side, on the optical axis (quotient 0 / z = 0: pixel (0, 0))
    def axis(zs):
        return [(0.0, 0.0, float(z)) for z in zs]
    z1 = [1.0, 1.125, below(1.125), above(1.125), 0.875, below(0.875), above(0.875), 1.0625, 1.25, 0.5]
    z0 = [0.125, below(0.125), above(0.125), -0.125, -below(0.125), -above(0.125), 0.0625, -0.0625, 2.0 ** -126, 0.25]
    for thresh in (0.125, 0.0):
        add(f"thresh{thresh}_d1", None, None, 160, 120, intrinsics(1, 0, 0), pose(), 1.0, thresh, cam=axis(z1))
        add(f"thresh{thresh}_d0", None, None, 160, 120, intrinsics(1, 0, 0), pose(), 0.0, thresh, cam=axis(z0))
    t01 = F32(0.1)                                          # the default thresh: z - 0 against 0.1f
    add("thresh0.1_d0", None, None, 160, 120, intrinsics(1, 0, 0), pose(), 0.0, 0.1,
        cam=axis([t01, below(t01), above(t01), -t01, -below(t01), -above(t01)]))
    # NaN / +-inf / 0 depth at the hit pixel, at a z that a finite depth of 1 (or 0) accepts
    d = np.ones((120, 160), F32)
    special = {(10, 20): np.nan, (11, 20): np.inf, (12, 20): -np.inf, (13, 20): 0.0, (119, 159): np.nan, (0, 0): np.inf}
    for (r, c), v in special.items():
        d[r, c] = v
    q = np.array([(c + 0.5, r + 0.5) for r, c in special] + [(21.5, 10.5), (20.5, 14.5)], F64)
    for z in (1.0, 1 / 16):
        add(f"depth_special_z{z}", q, z, 160, 120, intrinsics(1, 0, 0), pose(), d)
    # a 37 x 53 frame: f = 32, z = 2 -> quotients on quarters; every pixel centre against a depth map that walks through
    # the thresh boundary, and the borders
    w, h = 37, 53
    K = intrinsics(32, 18.5, 26.5)
    steps = np.array([-9, -8, -7, -1, 0, 1, 7, 8, 9], F64) / 64
    d = (2.0 + steps[(np.arange(h)[:, None] * 5 + np.arange(w)[None, :] * 3) % 9]).astype(F32)
    quarter = lambda n: [-1.25, -1.0, -0.75, -0.25, 0.0, 0.25, n - 0.25, float(n), n + 0.25]   # noqa: E731
    q = np.concatenate([np.array([(c + 0.5, r + 0.5) for r in range(h) for c in range(w)], F64),
                        cross(w, h, quarter(w), quarter(h))])
    add("frame_37x53", q, 2.0, w, h, K, pose((1, 0, 2), (-1, 1, 1), (-0.75, 2.0, 0.5)), d)
    add("frame_37x53_thresh0", q[::7], 2.0, w, h, K, pose(), d, 0.0)
    # a 1 x 1 frame (as [1, 1, 1]: the reference squeezes a leading axis of one, which a bare [1, 1] map would lose)
    v = [-1.0, above(-1), -0.5, 0.0, 0.5, below(1), 1.0, 2.0]
    add("frame_1x1", np.array([(x, y) for x in v for y in v], F64), 1.0, 1, 1, intrinsics(1, 0, 0), pose(), 1.0,
        squeeze=True)
    return out


def check_exact(c):
    """The float32 chain rounded after every operation equals the float64 one (so it is exact), where it is finite and z is
    a power of two; the depth coordinate is exact everywhere."""
    K4 = np.eye(4, dtype=F32)
    K4[:c["K"].shape[0], :c["K"].shape[1]] = c["K"]
    p = c["points"]

    def chain(m, x, t):
        m = m.astype(t)
        x = x.astype(t)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.stack([((m[r, 0] * x[:, 0] + m[r, 1] * x[:, 1]) + m[r, 2] * x[:, 2]) + m[r, 3] for r in range(3)], 1)
    i32, i64 = chain(K4, chain(c["w2c"], p, F32), F32), chain(K4, chain(c["w2c"], p, F64), F64)
    fin = np.isfinite(i64).all(1)
    assert np.array_equal(i32[fin].astype(F64), i64[fin]), c["name"]
    z = i64[:, 2]
    with np.errstate(invalid="ignore"):
        pow2 = fin & (z != 0) & (np.abs(np.frexp(np.where(fin, z, 1.0))[0]) == 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        q32, q64 = i32[:, :2] / i32[:, 2:], i64[:, :2] / i64[:, 2:]
    assert np.array_equal(q32[pow2].astype(F64), q64[pow2]), c["name"]
    on_axis = fin & (i64[:, 0] == 0) & (i64[:, 1] == 0)
    assert (pow2 | on_axis | ~fin | (z == 0)).all(), c["name"]


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ref_import.setup()
    import projection as RP                                 # the reference's projection.py, unmodified
    cs = cases()
    out = dict(n_cases=np.int64(len(cs)))
    total = 0
    for j, c in enumerate(cs):
        check_exact(c)
        proj = RP.Projection(torch.from_numpy(c["K"]), thresh=float(c["thresh"]))
        i2, i3 = proj.projection(torch.from_numpy(c["points"]), torch.from_numpy(c["depth"]), torch.from_numpy(c["w2c"]))
        i2, i3 = i2.numpy(), i3.numpy()
        n = len(c["points"])
        assert (np.diff(i3) > 0).all() and i2.min(initial=0) >= 0 and i2.max(initial=0) < 256
        keep = np.zeros(n, bool)
        keep[i3] = True
        out.update({f"{j}/name": np.array(c["name"]), f"{j}/points": c["points"], f"{j}/depth": c["depth"],
                    f"{j}/world2camera": c["w2c"], f"{j}/intrinsics": c["K"], f"{j}/thresh": c["thresh"],
                    f"{j}/keep": np.packbits(keep), f"{j}/inds2d": i2.astype(np.uint8)})
        total += n
        print(f"{c['name']:24s} points {n:5d} kept {len(i3):5d}")
    save_deterministic(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", total, "points")


if __name__ == "__main__":
    main()
