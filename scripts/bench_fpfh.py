"""FPFH descriptors (registration.compute_fpfh_feature_batch) on one GPU: prints ONE JSON line.  Device events around every
call, inputs already on the device, median [min, max] of --reps calls after one warm-up.

  clouds   : 2 x 120 000-point KITTI-shaped clouds (bench_icp_plane's undulating ground with two walls) and B = 64 shell
             clouds of 5 000 points.  For each, the FPFH radius is the first of a short list whose mean list length k (max_nn =
             100) lies in 50..100; it is printed with that mean.
  timed    : "normals+fpfh" -- compute_fpfh_feature_batch(normals=None): cell grid and normals (30 neighbours, half the FPFH
             radius) and cell grid and FPFH, from uploaded points to descriptors; "fpfh" -- the same with the normals given;
             "normals" -- estimate_normals_batch alone on the same input, the yardstick beside them.
  register : a synthetic pair (a bumpy surface of 5 000 points, its copy under a random pose with 1 mm noise, rows permuted)
             registered from FPFH alone: compute_fpfh_feature_batch, then register_batch; the pose error is printed.

There is no earlier implementation and no open3d timing for these inputs: the numbers are a record, not a speed-up."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import registration as REG  # noqa: E402
from scripts.bench_icp_plane import street  # noqa: E402
from tests import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)

MAX_NN = 100


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(out)), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3)}


def setting(clouds, radii, reps):
    pick = None
    for r in radii:
        cnt = REG.compute_fpfh_feature_batch(clouds, r, MAX_NN, normal_radius=0.5 * r, trace=True)[1]
        k = float(torch.cat(cnt).float().mean())
        pick = (r, k)
        if 50.0 <= k <= 100.0:
            break
    r, k = pick
    if not 50.0 <= k <= 100.0:
        raise SystemExit(f"no radius of {radii} gives a mean k in 50..100 (last: {r} -> {k:.1f})")
    nrm = REG.estimate_normals_batch(clouds, 0.5 * r, 30)
    return {"radius": r, "max_nn": MAX_NN, "k_mean": round(k, 2), "normal_radius": 0.5 * r, "normal_max_nn": 30,
            "normals+fpfh": timed(lambda: REG.compute_fpfh_feature_batch(clouds, r, MAX_NN, normal_radius=0.5 * r), reps),
            "fpfh": timed(lambda: REG.compute_fpfh_feature_batch(clouds, r, MAX_NN, normals=nrm), reps),
            "normals": timed(lambda: REG.estimate_normals_batch(clouds, 0.5 * r, 30), reps)}


def bumpy_pair(seed, n, noise=0.001):
    """A surface without symmetry over 4 m x 4 m and its copy under a random pose -> src, tgt (float32, rows permuted), T_gt,
    and the two viewpoints (one point above the surface, moved with it) that orient the normals alike."""
    rng = np.random.RandomState(seed)
    x, y = rng.rand(n) * 4.0, rng.rand(n) * 4.0
    z = 0.5 * np.sin(1.9 * x + 0.3) * np.cos(1.3 * y) + 0.3 * np.sin(2.7 * y + 1.0) + 0.05 * x * y + 0.2 * np.cos(3.1 * x * y / 4.0)
    src = np.stack([x, y, z], 1)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = RR.random_rotation(rng), rng.rand(3) - 0.5
    tgt = src @ T[:3, :3].T + T[:3, 3] + noise * rng.randn(n, 3)
    view = np.array([2.0, 2.0, 30.0])
    return src.astype(np.float32), tgt[rng.permutation(n)].astype(np.float32), T, np.stack([view, T[:3, :3] @ view + T[:3, 3]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--kitti-n", type=int, default=120000, help="0: skip the KITTI-shaped clouds")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "fpfh", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    if a.kitti_n:
        src, tgt, _ = street(77, a.kitti_n)
        out[f"clouds_2x{a.kitti_n}"] = setting([torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)],
                                               (0.6, 0.7, 0.8, 1.0, 0.5, 0.4), a.reps)
    clouds = [torch.from_numpy(RR.registration_pair(1000 + b, n=a.n, outliers=0.0, c=1, noise=0.003, shape="shell")[1]).to(dev)
              for b in range(a.batch)]
    out[f"clouds_{a.batch}x{a.n}"] = setting(clouds, (0.3, 0.35, 0.4, 0.25, 0.5, 0.2), a.reps)

    src, tgt, T_gt, views = bumpy_pair(5, a.n)
    r = 0.3
    fs, ft = REG.compute_fpfh_feature_batch([src, tgt], r, MAX_NN, normal_radius=0.5 * r, viewpoints=views)
    res = REG.register_batch([src], [tgt], [fs], [ft], distance_threshold=0.05, seeds=1)
    rot, trans = RR.pose_error(res.matrices[0], T_gt)
    out["register_from_fpfh"] = {"points": a.n, "radius": r, "distance_threshold": 0.05, "fitness": round(float(res.fitness[0]), 4),
                                 "rot_deg": float(f"{rot:.4g}"), "trans_m": float(f"{trans:.4g}")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
