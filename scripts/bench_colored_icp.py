"""Colored ICP beside point-to-plane ICP (registration.colored_icp_batch, refine_batch) on one GPU: prints ONE JSON line.
Device events around every call, inputs already on the device, one warm-up, then the median [min, max] of --reps calls; the
estimators take turns inside every repetition, in one process, on the same coloured pairs.

  scripts/bench_gicp.py's inputs with a smooth colour field on their surfaces: 64 pairs of 5 000 / 5 000 points (2 m cube
  shells, 3 mm noise, d = 0.05, 30 iterations, started 2 degrees and 3 cm off the ground truth), and ONE 120 000 / 120 000 pair
  (an undulating 40 m x 40 m ground with two walls, 5 mm noise, d = 0.2, 200 iterations, started 0.5 degrees and 0.1 m off).
  Both estimators estimate the targets' normals in the call (radius 0.15 / 0.5, 30 neighbours); colored ICP also builds the
  targets' colour gradients in the call (radius 2 d, 30 neighbours, lambda_geometric = 0.968).  Two more rows,
  "..._normals_given", pass the same normals in (estimated once, outside the timing).  "gradients" is
  color_gradients_batch alone on the targets with those normals: the grid at 2 d and the gradient kernel.
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
from scripts.bench_gicp import one  # noqa: E402
from scripts.bench_icp_plane import errors, off_by, street  # noqa: E402   (the same pairs and starts)
from tests import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)


def texture(pts, scale):
    """A smooth RGB field of wavelength about 2 scale on points in the source's frame -> float64 [n,3] in [0, 1]."""
    x, y, z = (np.asarray(pts, np.float64)[:, e] / scale for e in range(3))
    return np.stack([0.5 + 0.3 * np.sin(4.0 * x + 0.5) * np.cos(3.0 * y + z), 0.5 + 0.3 * np.cos(3.5 * y - 2.0 * z) * np.sin(2.0 * x + 1.0),
                     0.5 + 0.2 * np.sin(3.0 * z + 2.0 * x) + 0.2 * np.cos(2.5 * y)], 1)


def coloured(src, tgt, T_gt, scale, dev):
    """The pair on the device with the texture on its surface: the targets take the colour of their place in the source's frame."""
    back = (tgt.astype(np.float64) - T_gt[:3, 3]) @ T_gt[:3, :3]
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return on(src), on(tgt), on(texture(src, scale)), on(texture(back, scale))


def turns(src, tgt, cs, ct, start, gts, d, mi, radius, reps):
    nt = REG.estimate_normals_batch(tgt, radius, 30)
    calls = {
        "colored": lambda: REG.colored_icp_batch(src, tgt, cs, ct, start, d, max_iteration=mi, normal_radius=radius),
        "point_to_plane": lambda: REG.refine_batch(src, tgt, start, d, max_iteration=mi, estimation="point_to_plane",
                                                   normal_radius=radius),
        "colored_normals_given": lambda: REG.colored_icp_batch(src, tgt, cs, ct, start, d, max_iteration=mi, tgt_normals=nt),
        "point_to_plane_normals_given": lambda: REG.refine_batch(src, tgt, start, d, max_iteration=mi, estimation="point_to_plane",
                                                                 tgt_normals=nt),
        "gradients": lambda: REG.color_gradients_batch(tgt, ct, nt, 2.0 * d, 30),
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
        row[name] = {"ms_per_call": round(med, 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3)}
        if name != "gradients":
            row[name].update({"updates_mean": round(float(res.iterations.mean()), 2), "updates_max": int(res.iterations.max()),
                              "ms_per_update": round(med / (int(res.iterations.max()) + 1), 4),
                              "fitness": round(float(res.fitness.mean()), 4), "error_after": errors(res.matrices, gts)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="64")
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--kitti-n", type=int, default=120000, help="0: skip the KITTI-shaped pair")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    out = {"metric": "colored_icp", "device": torch.cuda.get_device_name(0), "reps": a.reps, "lambda_geometric": 0.968}
    pairs, gts, starts = [], [], []
    for b in range(max(batches)):
        src, tgt, _, _, T_gt = RR.registration_pair(1000 + b, n=a.n, outliers=0.0, c=1, noise=0.003, shape="shell")
        pairs.append(coloured(src, tgt, T_gt, 1.0, dev))
        gts.append(T_gt)
        starts.append(off_by(T_gt, 2.0, 0.03, b))
    for B in batches:
        start = torch.from_numpy(np.stack(starts[:B])).to(dev)
        out[f"refine_{a.n}_B{B}"] = turns(*([p[e] for p in pairs[:B]] for e in range(4)), start, gts[:B], 0.05, 30, 0.15, a.reps)
    if a.kitti_n:
        src, tgt, T_gt = street(77, a.kitti_n)
        s, t, cs, ct = coloured(src, tgt, T_gt, 10.0, dev)
        start = torch.from_numpy(off_by(T_gt, 0.5, 0.1, 5)[None]).to(dev)
        out[f"refine_{a.kitti_n}_B1"] = turns([s], [t], [cs], [ct], start, [T_gt], 0.2, 200, 0.5, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
