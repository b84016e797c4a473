"""Normal estimation and the two ICP estimators (registration.estimate_normals_batch, refine_batch) on one GPU: prints ONE
JSON line.  Device events around every call, inputs already on the device, the median of --reps calls after one warm-up.

  normals : 2 x 120 000-point KITTI-shaped clouds (radius 0.5, 30 neighbours) and B = 64 clouds of 5 000 points (radius
            0.15, 30 neighbours): ms per call, and the mean neighbour count.
  refine  : the same pairs through refine_batch(estimation="point_to_point") and ("point_to_plane", normals estimated in
            the call): 5 000 / 5 000 points (2 m cube shells, 3 mm noise, d = 0.05, 30 iterations, started 2 degrees and
            3 cm off the ground truth) at B = 1, 16, 64, and ONE 120 000 / 120 000 pair (an undulating 40 m x 40 m ground
            with two walls, 5 mm noise, d = 0.2, 200 iterations, started 0.5 degrees and 0.1 m off).  Per setting and
            estimator: ms per call, updates applied, pose error before and after.

The point-to-point rows are the numbers to hold the point-to-plane rows against (same process, same pairs); there is no
open3d timing for these inputs, so nothing here is a speed-up over the reference."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import registration as REG  # noqa: E402
from tests import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)


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
    return float(np.median(out))


def errors(mats, gts):
    e = np.array([RR.pose_error(T, G) for T, G in zip(mats, gts)])
    return {"rot_deg": float(f"{e[:, 0].mean():.4g}"), "trans_m": float(f"{e[:, 1].mean():.4g}")}


def off_by(T_gt, deg, shift, seed):
    rng = np.random.RandomState(seed)
    axis = rng.randn(3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    th = np.radians(deg)
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    t = rng.randn(3)
    D[:3, 3] = shift * t / np.linalg.norm(t)
    return D @ T_gt


def street(seed, n, noise=0.005):
    """A KITTI-shaped pair: an undulating 40 m x 40 m ground (70 % of the points) and two perpendicular 3 m walls, the
    target the source's image under a known pose plus noise, in another order -> src, tgt (float32), T_gt."""
    rng = np.random.RandomState(seed)
    u = rng.rand(n, 2) * 40.0 - 20.0
    kind = rng.rand(n)
    pts = np.stack([u[:, 0], u[:, 1], 0.3 * np.sin(u[:, 0] / 4.0) * np.cos(u[:, 1] / 5.0)], 1)
    a = kind > 0.7
    pts[a] = np.stack([u[a, 0], np.full(a.sum(), 12.0), (u[a, 1] + 20.0) * 0.075], 1)
    b = kind > 0.85
    pts[b] = np.stack([np.full(b.sum(), -15.0), u[b, 0], (u[b, 1] + 20.0) * 0.075], 1)
    T = np.eye(4)
    th = np.radians(3.0)
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    T[:3, 3] = [1.0, 0.3, 0.05]
    tgt = pts @ T[:3, :3].T + T[:3, 3] + noise * rng.randn(n, 3)
    return pts.astype(np.float32), tgt[rng.permutation(n)].astype(np.float32), T


def both(src, tgt, start, gts, d, mi, radius, reps):
    row = {}
    for name, kw in (("point_to_point", {}), ("point_to_plane", dict(estimation="point_to_plane", normal_radius=radius))):
        call = lambda: REG.refine_batch(src, tgt, start, d, max_iteration=mi, **kw)
        res = call()
        row[name] = {"ms_per_call": round(timed(call, reps), 3), "updates_mean": round(float(res.iterations.mean()), 2),
                     "updates_max": int(res.iterations.max()), "fitness": round(float(res.fitness.mean()), 4),
                     "error_after": errors(res.matrices, gts)}
    row["error_before"] = errors(start.cpu().numpy(), gts)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--kitti-n", type=int, default=120000, help="0: skip the KITTI-shaped clouds")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    out = {"metric": "icp_point_to_plane", "device": torch.cuda.get_device_name(0), "reps": a.reps}

    pairs, gts, starts = [], [], []
    for b in range(max(batches + [64])):
        src, tgt, _, _, T_gt = RR.registration_pair(1000 + b, n=a.n, outliers=0.0, c=1, noise=0.003, shape="shell")
        pairs.append((torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)))
        gts.append(T_gt)
        starts.append(off_by(T_gt, 2.0, 0.03, b))
    clouds = [p[1] for p in pairs[:64]]
    cnt = REG.estimate_normals_batch(clouds, 0.15, 30, trace=True)[1]
    out["normals_64x%d" % a.n] = {"radius": 0.15, "max_nn": 30, "neighbours_mean": round(float(torch.cat(cnt).float().mean()), 2),
                                  "ms_per_call": round(timed(lambda: REG.estimate_normals_batch(clouds, 0.15, 30), a.reps), 3)}
    for B in batches:
        start = torch.from_numpy(np.stack(starts[:B])).to(dev)
        out[f"refine_{a.n}_B{B}"] = both([p[0] for p in pairs[:B]], [p[1] for p in pairs[:B]], start, gts[:B], 0.05, 30, 0.15,
                                         a.reps)
    if a.kitti_n:
        src, tgt, T_gt = street(77, a.kitti_n)
        s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
        cnt = REG.estimate_normals_batch([s, t], 0.5, 30, trace=True)[1]
        out["normals_2x%d" % a.kitti_n] = {"radius": 0.5, "max_nn": 30, "neighbours_mean": round(float(torch.cat(cnt).float().mean()), 2),
                                           "ms_per_call": round(timed(lambda: REG.estimate_normals_batch([s, t], 0.5, 30), a.reps), 3)}
        start = torch.from_numpy(off_by(T_gt, 0.5, 0.1, 5)[None]).to(dev)
        out[f"refine_{a.kitti_n}_B1"] = both([s], [t], start, [T_gt], 0.2, 200, 0.5, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
