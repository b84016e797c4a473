"""tests/golden/projection.npz: PCR-CG's RGB-D projection from the UNMODIFIED reference (ref:projection.py, build container
only), and SuperGlue valid maps.

Projection part: Projection(intrinsics).projection(points, depth_map, world2camera) of the reference, run as it ships, on
  - 6 000 points sampled from each asset fragment (ref:assets/cloud_bin_21.pth, cloud_bin_34.pth), image 1 under the
    identity world2camera and image 2 under a world2camera composed the way the loader composes it
    (pcrcg_amd.synthetic.second_world2camera), the depth maps z-buffer-rendered from the whole fragment with noise and
    dropped pixels (pcrcg_amd.synthetic.render_depth) and rounded to float16 values;
  - an edge-case cloud (edge_case()): z = 0, z < 0, quotients in (-1, 0) and a few ulps either side of the pixel borders,
    huge and non-finite coordinates, zero-depth pixels, |z - d| a few ulps either side of 0.1f, a [1, H, W] depth map.
  These are the guards of correct code: nothing here is meant to fault.
Stored per case: its cloud, depth, world2camera, and the reference's result as a keep mask over the points (inds3d =
the kept indices, ascending) and inds2d in bytes; the intrinsics (3x3, as the loader has them) once.  Everything is
stored losslessly in a compressed npz; tests/projection_ref.load_fixture() rebuilds the tensors.

Valid-map part: NOT the reference's code run -- its painting loop lives inside the data loader's __getitem__ and needs the
dataset on disk.  The maps come from tests/projection_ref.paint_valid_maps, a numpy restatement of ref:datasets/indoor.py:
284-299 written for this project that paints with numpy's own slice assignment (so numpy's slice rules are the ones
pinned), on SuperGlue-like matches with keypoints near and past the borders."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

OUT = os.path.join(ref_import.REPO, "tests", "golden", "projection.npz")
SAMPLE = 6000          # points sampled from each asset fragment
sys.path.insert(0, os.path.join(ref_import.REPO, "tests"))


def _ulps(v, k):
    """float32 values k ulps either side of v (v included)."""
    out, lo, hi = [np.float32(v)], np.float32(v), np.float32(v)
    for _ in range(k):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


def edge_case(K):
    """Points against a 120 x 160 depth map, world2camera = identity: every guard of the projection."""
    fx, cx, cy = float(K[0, 0]), float(K[0, 2]), float(K[1, 2])
    h, w = 120, 160
    depth = np.ones((h, w), np.float32)
    depth[:, :8] = 0.0                                  # zero (missing) depth pixels
    depth[50:70, 100:110] = 0.0
    pts = []

    def at(qx, qy, z):                                  # a point whose quotients are about (qx, qy) at depth z
        pts.append([(qx - cx) * z / fx, (qy - cy) * z / fx, z])

    for z in (0.0, -0.0):                               # z = 0: 0/0 and x/0
        pts += [[0.0, 0.0, z], [0.3, -0.2, z], [-1.0, 1.0, z]]
    for z in (-0.05, -0.09, -0.5, -2.0):                # behind the camera, on missing and on real depth
        at(104.0, 60.0, z)
        at(3.5, 30.5, z)
        at(40.0, 20.0, z)
    for q in (-0.999, -0.5, -1e-7, -0.0, 1e-7, 0.5, 0.999):   # quotients in (-1, 0) and near 0 -> pixel 0 on either axis
        at(q, 60.5, 1.0)
        at(80.5, q, 1.0)
        at(q, 60.5, 0.05)
    for v in [*_ulps(-1.0, 6), *_ulps(1.0, 6), *_ulps(159.0, 6), *_ulps(160.0, 6), *_ulps(80.0, 4)]:
        for z in (1.0, 1.05, 0.07):                     # column borders, then row borders
            at(float(v), 60.5, z)
        for z in (1.0, 0.95):
            at(80.5, float(v) * 119.0 / 160.0 if abs(float(v)) > 1.5 else float(v), z)
    for v in _ulps(119.0, 6) + _ulps(120.0, 6):
        at(30.5, float(v), 1.0)
    for z in _ulps(np.float32(1.0) + np.float32(0.1), 8):   # |z - d| around 0.1f with d = 1 (z - 1 is exact there)
        at(30.5, 30.5, float(z))
    for z in _ulps(0.1, 8):                             # |z - 0| around 0.1f on missing pixels, in front and behind
        at(3.5, 40.5, float(z))
        at(104.5, 60.5, float(z))
        at(104.5, 60.5, -float(z))
    for big in (1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan):   # huge and non-finite coordinates
        pts += [[big, 0.0, 1.0], [0.0, big, 1.0], [0.0, 0.0, big], [big, big, big], [1e-3, 1e-3, big]]
    p = np.asarray(pts, np.float64).astype(np.float32)
    return p, depth[None]                               # a [1, H, W] map: the reference squeezes it


def valid_cases(rng):
    """SuperGlue-like matches with keypoints near and past the borders, and the maps painted from them.  Stored as the
    number of the valid match that paints each pixel last (painted with the values 1..n_valid: which match paints a pixel
    does not depend on the values), from which the maps are confidence[valid][idx - 1], 0 where idx = 0."""
    from projection_ref import paint_valid_maps
    from pcrcg_amd import synthetic as S
    cases = []
    for n0, n1 in ((400, 450), (37, 20)):
        sg = S.superglue_like(rng, n0, n1)
        edge = np.array([[0.0, 0.0], [4.99, 3.0], [5.0, 119.9], [-3.0, 60.0], [159.99, 119.99], [160.0, 0.0], [4.2, 4.7],
                         [-0.5, 5.5], [155.0, 115.0], [170.0, 130.0], [-7.0, -7.0], [2.0, 200.0]], np.float32)
        sg["keypoints0"][:len(edge)] = edge
        sg["keypoints1"][:len(edge)] = edge[::-1]
        sg["matches"][:len(edge)] = np.arange(len(edge))
        order = np.arange(1, int((sg["matches"] > -1).sum()) + 1, dtype=np.float32)
        tag = np.zeros(n0, np.float32)
        tag[sg["matches"] > -1] = order
        src_idx, tgt_idx = paint_valid_maps(sg["keypoints0"], sg["keypoints1"], sg["matches"], tag, 5)
        sg["src_idx"], sg["tgt_idx"] = src_idx.astype(np.int16), tgt_idx.astype(np.int16)
        cases.append(sg)
    return cases


def main():
    ref_import.setup()
    import projection as RP                             # /root/reference/projection.py, unmodified
    from pcrcg_amd import synthetic as S
    rng = np.random.RandomState(7)
    K = S.INTRINSICS_160
    clouds, cases = {}, []
    for name in ("cloud_bin_21", "cloud_bin_34"):
        full = np.asarray(torch.load(os.path.join(ref_import.REF, "assets", name + ".pth"), weights_only=False), np.float32)
        # SAMPLE points of the fragment in their original order (the fixture stays small); the depth maps are rendered
        # from the whole fragment, so the sampled points behind its front surface are rejected as they would be
        clouds[name] = full[np.sort(rng.permutation(len(full))[:SAMPLE])]
        w2c1 = np.eye(4, dtype=np.float32)
        w2c2 = S.second_world2camera(np.eye(4), S._pose(rng), w2c1)
        for tag, w2c in (("identity", w2c1), ("composed", w2c2)):
            depth = S.render_depth(full, w2c, K, rng=rng).astype(np.float16)     # float16 values: stored exactly
            cases.append(dict(name=f"{name}/{tag}", cloud=name, depth=depth, world2camera=w2c))
    clouds["edge"], d = edge_case(K)
    cases.append(dict(name="edge", cloud="edge", depth=d.astype(np.float16), world2camera=np.eye(4, dtype=np.float32)))
    out = dict(intrinsics=K, window=np.int64(5), n_cases=np.int64(len(cases)))
    out.update({f"cloud/{k}": v for k, v in clouds.items()})
    for j, c in enumerate(cases):
        pts = torch.from_numpy(clouds[c["cloud"]])
        depth = torch.from_numpy(c["depth"].astype(np.float32))
        i2, i3 = RP.Projection(torch.from_numpy(K)).projection(pts, depth, torch.from_numpy(c["world2camera"]))
        i2, i3 = i2.numpy(), i3.numpy()
        # the reference's inds3d ascend (boolean masks) and its pixels fit a byte: a keep mask and uint8 pixels are lossless
        assert (np.diff(i3) > 0).all() and i2.min(initial=0) >= 0 and i2.max(initial=0) < 256
        keep = np.zeros(len(pts), bool)
        keep[i3] = True
        out.update({f"{j}/name": np.array(c["name"]), f"{j}/cloud": np.array(c["cloud"]), f"{j}/depth": c["depth"],
                    f"{j}/world2camera": c["world2camera"], f"{j}/keep": np.packbits(keep), f"{j}/inds2d": i2.astype(np.uint8)})
        print(c["name"], tuple(pts.shape), "kept", len(i3))
    for j, v in enumerate(valid_cases(rng)):
        out.update({f"valid{j}/{k}": val for k, val in v.items()})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
