"""The 3DMatch / 3DLoMatch registration benchmark end to end -- the project's equivalent of the reference's run_ransac.sh.

The reference loops over n_points = 250 .. 5000 calling a scripts/evaluate_predator.py that its tree does not contain.
This script's loop is the tester's sample-then-register loop (ref:lib/tester.py:140-169), not a restatement of that
file: for every `--n_points`, the tester's `{idx}.pth` records (tester.test_record) are loaded in natural order, each
record is sampled on the host generator (overlap x saliency, source then target) and all pairs are registered in one
batched RANSAC (tester.register_records -> registration.register_batch).  The poses are written per scene as
`{exp_dir}/{n_points}/{scene}/est.log` -- the records taken in the order of the scenes of `--gt_folder` (sorted) and
of the pairs of each scene's gt.log -- and scored with benchmark.benchmark, which writes `{exp_dir}/{n_points}/result`.

  python scripts/evaluate_registration.py --source_path snapshot/.../test/pth --gt_folder configs/benchmarks/3DMatch \\
      --exp_dir snapshot/.../est_traj [--n_points 250 500 1000 2500 5000]
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import benchmark as BM  # noqa: E402
from pcrcg_amd import tester  # noqa: E402


def natural_key(name):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source_path", required=True, help="folder of the tester's {idx}.pth records")
    ap.add_argument("--gt_folder", required=True, help="configs/benchmarks/<3DMatch|3DLoMatch>: one folder per scene")
    ap.add_argument("--exp_dir", required=True, help="where est.log, result and flag.npy go (one folder per n_points)")
    ap.add_argument("--n_points", type=int, nargs="+", default=[250, 500, 1000, 2500, 5000])
    ap.add_argument("--distance_threshold", type=float, default=0.05)
    ap.add_argument("--ransac_n", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0, help="np.random seed before each sampling pass")
    a = ap.parse_args()

    files = sorted((f for f in os.listdir(a.source_path) if f.endswith(".pth")), key=natural_key)
    records = [torch.load(os.path.join(a.source_path, f)) for f in files]
    scenes = sorted(os.listdir(a.gt_folder))
    keys = [BM.read_trajectory(os.path.join(a.gt_folder, s, "gt.log"))[0] for s in scenes]
    if sum(len(k) for k in keys) != len(records):
        raise SystemExit(f"{len(records)} records for {sum(len(k) for k in keys)} gt pairs in {a.gt_folder}")
    summary = {}
    for n_points in a.n_points:
        np.random.seed(a.seed)
        poses = tester.register_records(records, n_points=n_points, distance_threshold=a.distance_threshold,
                                        ransac_n=a.ransac_n)
        out_dir = os.path.join(a.exp_dir, str(n_points))
        o = 0
        for scene, k in zip(scenes, keys):
            BM.write_est_trajectory(out_dir, scene, k, np.stack(poses[o:o + len(k)]))
            o += len(k)
        res = BM.benchmark(out_dir, a.gt_folder)
        summary[n_points] = {"mean_recall": res["mean_recall"], "mean_precision": res["mean_precision"]}
        print(n_points, open(os.path.join(out_dir, "result")).read(), sep="\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
