"""The ModelNet / ModelLoNet evaluation end to end -- ModelnetTester.test (ref:lib/tester.py:343-436) on stored records.

A record is the tester's dict (tester.test_record: pcd, feats, overlaps, saliency, len_src, rot, trans) plus `sample`,
the loader's dict of transform_gt, points_src, points_ref and points_raw.  The `{idx}.pth` records of --source_path are
loaded in natural order, sampled to 450 points on the host generator (overlap x saliency, source then target),
registered in one batched RANSAC (0.02, ransac_n 3) and scored by ONE batched metrics call
(tester.evaluate_modelnet_records -> modelnet.compute_metrics -> pcrcg_chamfer_batch).  Prints the reference's
"rotation range in data" and print_metrics lines, then one JSON line with the summary.

  python scripts/evaluate_modelnet.py --source_path snapshot/.../test/pth [--out metrics.npz] [--sampler device]

--sampler device draws the interest points on the GPU in one launch (registration.sample_batch; record b with sample seed
--seed + b) instead of on the host generator.
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import modelnet, tester  # noqa: E402


def natural_key(name):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source_path", required=True, help="folder of {idx}.pth ModelNet records")
    ap.add_argument("--n_points", type=int, default=450)
    ap.add_argument("--distance_threshold", type=float, default=0.02)
    ap.add_argument("--ransac_n", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0, help="np.random seed before the sampling pass")
    ap.add_argument("--sampler", choices=("host", "device"), default="host",
                    help="host: np.random.choice as the reference; device: one GPU launch, sample seeds --seed + record index")
    ap.add_argument("--out", help="optional .npz for the poses and the per-pair metrics")
    a = ap.parse_args()
    files = sorted((f for f in os.listdir(a.source_path) if f.endswith(".pth")), key=natural_key)
    if not files:
        raise SystemExit(f"no .pth records in {a.source_path}")
    records = [torch.load(os.path.join(a.source_path, f)) for f in files]
    np.random.seed(a.seed)
    poses, metrics, summary = tester.evaluate_modelnet_records(records, n_points=a.n_points, distance_threshold=a.distance_threshold,
                                                               ransac_n=a.ransac_n, sampler=a.sampler,
                                                               sample_seeds=[(a.seed + b) % (1 << 23) for b in range(len(records))])
    print("Rotation range in data: {}(avg), {}(max)".format(summary["rotation_mean"], summary["rotation_max"]))
    modelnet.print_metrics(summary, title="Evaluation result (iter 0)")
    if a.out:
        np.savez(a.out, poses=np.stack(poses), **metrics)
    print(json.dumps({k: float(v) for k, v in summary.items()}))


if __name__ == "__main__":
    main()
