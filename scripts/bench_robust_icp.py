"""Point-to-plane ICP under the robust kernels (registration.robust_refine_batch; kernel None: refine_batch's own call) beside the
plain estimator on one GPU: prints ONE JSON line.  Device events around every call, inputs and normals already on the device,
one warm-up call per estimator, then --reps rounds in which the estimators TAKE TURNS on the same pairs (plain, L2, L1, Huber,
Cauchy, GM, Tukey; plain, ...), so that a drift of the machine touches all of them alike: median [min, max] ms per call.

  64 x 5 000 / 5 000 : scripts/bench_icp_plane.py's shell pairs (2 m cube shells, 3 mm noise, d = 0.05, 30 iterations, started
                       2 degrees and 3 cm off the ground truth), the targets' normals estimated once (radius 0.15) and passed in.
  1 x 120 000 / 120 000 : its KITTI-shaped street pair (5 mm noise, d = 0.2, 200 iterations, started 0.5 degrees and 0.1 m off),
                       normals at radius 0.5 passed in.

The kinds stop after different numbers of updates, and a call's time follows the number of evaluations that still have a live
pair, so beside ms per call every row has the mean and the largest number of updates and ms per update (ms per call over the
largest number of updates + 1: the evaluations the slowest pair ran).  That figure still holds a call's fixed part -- uploads,
the cell grid, and the launches past a pair's stop, which leave at once -- spread over fewer or more updates, so every shape is
measured a second time with both convergence bounds 0 and a cap of --fixed updates (`*_fixed`): there every estimator runs the
same number of evaluations and the ratio per call IS the ratio per update.  `ratio_*` is a kind's figure over the plain
estimator's of the same run; `plain_spread` is (max - min) / median of the plain rows, the run-to-run noise to hold the ratios
against."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import registration as REG  # noqa: E402
from scripts.bench_icp_plane import errors, off_by, street  # noqa: E402
from tests import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)

KERNELS = (("plain", None), ("L2", REG.L2Loss()), ("L1", REG.L1Loss()), ("Huber", REG.HuberLoss(0.005)),
           ("Cauchy", REG.CauchyLoss(0.005)), ("GM", REG.GMLoss(1e-4)), ("Tukey", REG.TukeyLoss(0.015)))


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), res


def turns(src, tgt, start, normals, gts, d, mi, reps, **bounds):
    calls = {name: (lambda k=k: REG.robust_refine_batch(src, tgt, start, d, k, max_iteration=mi, tgt_normals=normals, **bounds))
             for name, k in KERNELS}
    results = {name: fn() for name, fn in calls.items()}            # the warm-up of every estimator, and its result
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            times[name].append(one_call(fn)[0])
    rows = {}
    for name, res in results.items():
        t = np.array(times[name])
        evals = int(res.iterations.max()) + 1
        rows[name] = {"ms_per_call": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3),
                      "updates_mean": round(float(res.iterations.mean()), 2), "updates_max": int(res.iterations.max()),
                      "ms_per_update": round(float(np.median(t)) / evals, 4), "fitness": round(float(res.fitness.mean()), 4),
                      "error_after": errors(res.matrices, gts)}
    plain = rows["plain"]
    for name, row in rows.items():
        row["ratio_per_call"] = round(row["ms_per_call"] / plain["ms_per_call"], 4)
        row["ratio_per_update"] = round(row["ms_per_update"] / plain["ms_per_update"], 4)
    rows["plain_spread"] = round((plain["ms_max"] - plain["ms_min"]) / plain["ms_per_call"], 4)
    rows["error_before"] = errors(start.cpu().numpy(), gts)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--fixed", type=int, default=10, help="the cap of the runs in which every estimator applies the same number of updates")
    ap.add_argument("--kitti-n", type=int, default=120000, help="0: skip the KITTI-shaped pair")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "icp_robust_kernels", "device": torch.cuda.get_device_name(0), "reps": a.reps}

    src, tgt, gts, starts = [], [], [], []
    for b in range(a.pairs):
        s, t, _, _, T_gt = RR.registration_pair(1000 + b, n=a.n, outliers=0.0, c=1, noise=0.003, shape="shell")
        src.append(torch.from_numpy(s).to(dev))
        tgt.append(torch.from_numpy(t).to(dev))
        gts.append(T_gt)
        starts.append(off_by(T_gt, 2.0, 0.03, b))
    normals = REG.estimate_normals_batch(tgt, 0.15, 30)
    zero = dict(relative_fitness=0.0, relative_rmse=0.0)
    start = torch.from_numpy(np.stack(starts)).to(dev)
    out[f"{a.pairs}x{a.n}"] = turns(src, tgt, start, normals, gts, 0.05, 30, a.reps)
    out[f"{a.pairs}x{a.n}_fixed"] = turns(src, tgt, start, normals, gts, 0.05, a.fixed, a.reps, **zero)
    if a.kitti_n:
        s, t, T_gt = street(77, a.kitti_n)
        s, t = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
        normals = REG.estimate_normals_batch([t], 0.5, 30)
        start = torch.from_numpy(off_by(T_gt, 0.5, 0.1, 5)[None]).to(dev)
        out[f"1x{a.kitti_n}"] = turns([s], [t], start, normals, [T_gt], 0.2, 200, a.reps)
        out[f"1x{a.kitti_n}_fixed"] = turns([s], [t], start, normals, [T_gt], 0.2, a.fixed, a.reps, **zero)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
