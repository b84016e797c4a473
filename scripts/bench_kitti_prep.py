"""Preparing a KITTI pair on one GPU (pcrcg_amd/kitti.py): prints ONE JSON line.

Workload: scripts/bench_icp.py's KITTI-shaped pair -- two 120 000-point slab scans (40 m x 40 m x 0.6 m, 5 mm noise, a known
pose) -- at first_subsampling_dl = 0.3 m.  Inputs already on the device; every timed call includes its read-back; the median
of --reps calls after one warm-up:

  voxel_ms      : voxel_down_sample_batch on both scans (one library call, one read-back)
  prepare_ms    : prepare_pairs with `refined` given (down-sampling, correspondences, the dict; no ICP)
  numpy_ms      : the numpy restatement of the same down-sampling (tests/voxel_ref.py) on this host's CPU, both scans

The results are also compared (rows, bit for bit) before anything is timed.
Recorded on one MI355X (one run, median of 9, spread not measured): voxel_ms 0.244, prepare_ms 0.578,
numpy_ms 33.3 on that host's CPU; 46 450 / 42 770 rows, bit-identical to numpy, 541 282 correspondences.
open3d is not installable here, so there is NO open3d timing and nothing printed is a speed-up over the reference; the
numpy figure is a single-thread restatement, not open3d's C++."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import kitti, kitti_config  # noqa: E402
from tests import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)
from tests import voxel_ref as VR  # noqa: E402


def timed(fn, reps, sync):
    out = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n", type=int, default=120000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = kitti_config()
    src, tgt, _, _, T_gt = RR.registration_pair(77, n=a.n, outliers=0.0, c=1, noise=0.005, shape="slab")
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    voxel = cfg.first_subsampling_dl

    down = kitti.voxel_down_sample_batch([s, t], voxel)                                 # warm-up, and the comparison
    refs = [VR.voxel_down_sample(src, voxel), VR.voxel_down_sample(tgt, voxel)]
    same = all(d.cpu().numpy().tobytes() == r[0].tobytes() for d, r in zip(down, refs))
    item = kitti.prepare_pairs([s], [t], [T_gt], cfg, refined=[T_gt])[0]
    out = {"metric": "kitti_prep", "device": torch.cuda.get_device_name(0), "reps": a.reps, "n_points": a.n, "voxel": voxel,
           "rows": [int(d.shape[0]) for d in down], "bit_identical_to_numpy": bool(same),
           "n_correspondences": item["n_correspondences"]}
    out["voxel_ms"] = round(1e3 * timed(lambda: kitti.voxel_down_sample_batch([s, t], voxel), a.reps, True), 3)
    out["prepare_ms"] = round(1e3 * timed(lambda: kitti.prepare_pairs([s], [t], [T_gt], cfg, refined=[T_gt]), a.reps, True), 3)
    out["numpy_ms"] = round(1e3 * timed(lambda: [VR.voxel_down_sample(src, voxel), VR.voxel_down_sample(tgt, voxel)],
                                        min(a.reps, 3), False), 3)
    out["open3d_ms"] = None          # not measured: open3d is not installable here
    print(json.dumps(out))


if __name__ == "__main__":
    main()
