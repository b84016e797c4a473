"""Generalized ICP beside the two other ICP estimators (registration.generalized_icp_batch, refine_batch) on one GPU: prints
ONE JSON line.  Device events around every call, inputs already on the device, one warm-up, then the median [min, max] of
--reps calls; the three estimators take turns inside every repetition, in one process, on the same pairs.

  scripts/bench_icp_plane.py's inputs: 5 000 / 5 000 points (2 m cube shells, 3 mm noise, d = 0.05, 30 iterations, started
  2 degrees and 3 cm off the ground truth) at B = 1, 16, 64, and ONE 120 000 / 120 000 pair (an undulating 40 m x 40 m ground
  with two walls, 5 mm noise, d = 0.2, 200 iterations, started 0.5 degrees and 0.1 m off).  Point-to-plane and Generalized ICP
  estimate their normals in the call (radius 0.15 / 0.5, 30 neighbours; Generalized ICP on both clouds, epsilon = 1e-3).
  Two more rows, "..._normals_given", pass the same normals in (estimated once, outside the timing): the loops alone, without
  the one (point-to-plane) or two (generalized) normal estimations of the call.
  Per setting and row: ms per call, updates applied, pose error before and after; ms_per_update = the median over
  (the largest update count of the batch + 1) evaluations -- the launches that found a live pair.

There is no open3d timing for these inputs, so nothing here is a speed-up over the reference."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import registration as REG  # noqa: E402
from scripts.bench_icp_plane import errors, off_by, street  # noqa: E402   (the same pairs and starts)
from tests import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def three(src, tgt, start, gts, d, mi, radius, reps):
    ns, nt = REG.estimate_normals_batch(src, radius, 30), REG.estimate_normals_batch(tgt, radius, 30)
    calls = {
        "point_to_point": lambda: REG.refine_batch(src, tgt, start, d, max_iteration=mi),
        "point_to_plane": lambda: REG.refine_batch(src, tgt, start, d, max_iteration=mi, estimation="point_to_plane",
                                                   normal_radius=radius),
        "generalized": lambda: REG.generalized_icp_batch(src, tgt, start, d, max_iteration=mi, normal_radius=radius),
        "point_to_plane_normals_given": lambda: REG.refine_batch(src, tgt, start, d, max_iteration=mi, estimation="point_to_plane",
                                                                 tgt_normals=nt),
        "generalized_normals_given": lambda: REG.generalized_icp_batch(src, tgt, start, d, max_iteration=mi, src_normals=ns,
                                                                       tgt_normals=nt),
    }
    results = {name: call() for name, call in calls.items()}          # the warm-up, and the numbers
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            times[name].append(one(call))
    row = {"error_before": errors(start.cpu().numpy(), gts)}
    for name, res in results.items():
        t = np.array(times[name])
        med = float(np.median(t))
        row[name] = {"ms_per_call": round(med, 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3),
                     "updates_mean": round(float(res.iterations.mean()), 2), "updates_max": int(res.iterations.max()),
                     "ms_per_update": round(med / (int(res.iterations.max()) + 1), 4),
                     "fitness": round(float(res.fitness.mean()), 4), "error_after": errors(res.matrices, gts)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--kitti-n", type=int, default=120000, help="0: skip the KITTI-shaped pair")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    out = {"metric": "generalized_icp", "device": torch.cuda.get_device_name(0), "reps": a.reps, "epsilon": 1e-3}
    pairs, gts, starts = [], [], []
    for b in range(max(batches)):
        src, tgt, _, _, T_gt = RR.registration_pair(1000 + b, n=a.n, outliers=0.0, c=1, noise=0.003, shape="shell")
        pairs.append((torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)))
        gts.append(T_gt)
        starts.append(off_by(T_gt, 2.0, 0.03, b))
    for B in batches:
        start = torch.from_numpy(np.stack(starts[:B])).to(dev)
        out[f"refine_{a.n}_B{B}"] = three([p[0] for p in pairs[:B]], [p[1] for p in pairs[:B]], start, gts[:B], 0.05, 30, 0.15,
                                          a.reps)
    if a.kitti_n:
        src, tgt, T_gt = street(77, a.kitti_n)
        s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
        start = torch.from_numpy(off_by(T_gt, 0.5, 0.1, 5)[None]).to(dev)
        out[f"refine_{a.kitti_n}_B1"] = three([s], [t], start, [T_gt], 0.2, 200, 0.5, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
