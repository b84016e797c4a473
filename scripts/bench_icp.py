"""ICP refinement (registration.refine_batch) on one GPU, next to the RANSAC it follows: prints ONE JSON line.

Two settings, inputs already on the device, every timed call including its one read-back, the median of --reps calls:

  3dmatch : 5 000 / 5 000 points (scripts/bench_registration_batch.py's synthetic shell pairs, 50 % outlier descriptors,
            3 mm noise), d = 0.05, 30 iterations, started from register_batch's poses, at B = 1, 16, 64, 256.  Per B: ms per
            pair of refine_batch and of register_batch (same process, same pairs), their ratio, the iterations actually
            run and the mean pose error against ground truth before and after.
  kitti   : ONE pair of 120 000 / 120 000 points (a 40 m x 40 m x 0.6 m slab, 5 mm noise), d = 0.2, 200 iterations, started
            0.5 degrees and 0.1 m off the ground truth: ms per call, iterations run, pose error before and after.

Not measured yet: no MI355X run of this script has been recorded (DESIGN.md section 10 says the same).
No open3d timing exists for these inputs, so nothing here is a speed-up over the reference."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import registration as REG  # noqa: E402
from tests import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def errors(mats, gts):
    e = np.array([RR.pose_error(T, G) for T, G in zip(mats, gts)])
    return {"rot_deg": round(float(e[:, 0].mean()), 5), "trans_m": round(float(e[:, 1].mean()), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--kitti-n", type=int, default=120000, help="0: skip the KITTI-shaped pair")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    out = {"metric": "icp_refinement", "device": torch.cuda.get_device_name(0), "reps": a.reps}

    pairs, gts = [], []
    for b in range(max(batches)):
        src, tgt, f, g, T_gt = RR.registration_pair(1000 + b, n=a.n, outliers=0.5, noise=0.003, shape="shell")
        pairs.append([torch.from_numpy(x).to(dev) for x in (src, tgt, f, g)])
        gts.append(T_gt)
    row = {"n_points": a.n, "distance": 0.05, "max_iteration": 30}
    for B in batches:
        lists = [list(x) for x in zip(*pairs[:B])]
        seeds = list(range(B))
        reg = REG.register_batch(*lists, 0.05, 3, seeds=seeds)
        t_reg = timed(lambda: REG.register_batch(*lists, 0.05, 3, seeds=seeds), a.reps)
        res = REG.refine_batch(lists[0], lists[1], reg, 0.05, max_iteration=30)
        t_icp = timed(lambda: REG.refine_batch(lists[0], lists[1], reg, 0.05, max_iteration=30), a.reps)
        row[f"B{B}"] = {"icp_ms_per_pair": round(1e3 * t_icp / B, 4), "ransac_ms_per_pair": round(1e3 * t_reg / B, 4),
                        "icp_over_ransac": round(t_icp / t_reg, 4),
                        "iterations_mean": round(float(res.iterations.mean()), 2), "iterations_max": int(res.iterations.max()),
                        "fitness_before": round(float(reg.fitness.mean()), 4), "fitness_after": round(float(res.fitness.mean()), 4),
                        "error_before": errors(reg.matrices, gts[:B]), "error_after": errors(res.matrices, gts[:B])}
    out["3dmatch"] = row

    if a.kitti_n:
        src, tgt, _, _, T_gt = RR.registration_pair(77, n=a.kitti_n, outliers=0.0, c=1, noise=0.005, shape="slab")
        off = np.eye(4)
        th = np.radians(0.5)
        off[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        off[:3, 3] = [0.08, -0.06, 0.0]
        start = (off @ T_gt)[None]
        s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
        start_d = torch.from_numpy(start).to(dev)
        res = REG.refine_batch([s], [t], start_d, 0.2, max_iteration=200)
        t_icp = timed(lambda: REG.refine_batch([s], [t], start_d, 0.2, max_iteration=200), a.reps)
        out["kitti"] = {"n_points": a.kitti_n, "distance": 0.2, "max_iteration": 200, "ms_per_call": round(1e3 * t_icp, 3),
                        "iterations": int(res.iterations[0]), "fitness": round(float(res.fitness[0]), 4),
                        "inlier_rmse": round(float(res.inlier_rmse[0]), 5),
                        "error_before": errors(start, [T_gt]), "error_after": errors(res.matrices, [T_gt])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
