"""The 3DMatch / 3DLoMatch registration benchmark end to end -- the project's equivalent of the reference's run_ransac.sh.

The reference loops over n_points = 250 .. 5000 calling a scripts/evaluate_predator.py that its tree does not contain.
This script's loop is the tester's sample-then-register loop (ref:lib/tester.py:140-169), not a restatement of that
file: for every `--n_points`, the tester's `{idx}.pth` records (tester.test_record) are loaded in natural order, each
record is sampled on the host generator (overlap x saliency, source then target) and all pairs are registered in one
batched RANSAC (tester.register_records -> registration.register_batch).  The poses are written per scene as
`{exp_dir}/{n_points}/{scene}/est.log` -- the records taken in the order of the scenes of `--gt_folder` (sorted) and
of the pairs of each scene's gt.log -- and scored with benchmark.benchmark, which writes `{exp_dir}/{n_points}/result`.
With --inlier_ratio the same samples also give the inlier ratios against the records' ground truth
(tester.evaluate_records -> registration.inlier_ratio_batch, one batched call); the inlier ratio (IR) and feature-match
recall (FMR) lines of benchmark.feature_match_recall, without and with the mutual check, are appended to each `result`
and added to the summary.

  python scripts/evaluate_registration.py --source_path snapshot/.../test/pth --gt_folder configs/benchmarks/3DMatch \\
      --exp_dir snapshot/.../est_traj [--n_points 250 500 1000 2500 5000] [--inlier_ratio] [--sampler device] [--icp DIST]
      [--icp-estimation point_to_plane|generalized --normal-radius R]

--sampler device draws the interest points of all records on the GPU in one launch (registration.sample_batch: the same
distribution from its own seeded stream, record b with sample seed --seed + b) instead of on the host generator.
--icp DIST refines every RANSAC pose by point-to-point ICP on the record's full clouds with correspondence distance DIST
(registration.refine_batch); without it the poses are RANSAC's, as before.  --icp-estimation point_to_plane makes that
refinement point-to-plane, on target normals estimated with --normal-radius (required then) in the same call;
--icp-estimation generalized makes it Generalized ICP (registration.generalized_icp_batch) on the normals of both clouds,
estimated with --normal-radius (required too).
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
    ap.add_argument("--sampler", choices=("host", "device"), default="host",
                    help="host: np.random.choice as the reference; device: one GPU launch, sample seeds --seed + record index")
    ap.add_argument("--inlier_ratio", action="store_true", help="also report the inlier ratio and feature-match recall")
    ap.add_argument("--inlier_distance", type=float, default=0.1, help="inlier distance threshold of IR / FMR (m)")
    ap.add_argument("--fmr_threshold", type=float, default=0.05, help="inlier ratio above which a pair counts for FMR")
    ap.add_argument("--icp", type=float, default=None, metavar="DIST",
                    help="refine every pose by ICP on the full clouds with this correspondence distance (default: off)")
    ap.add_argument("--icp-estimation", choices=("point_to_point", "point_to_plane", "generalized"), default="point_to_point",
                    help="the estimator of --icp (default: point_to_point)")
    ap.add_argument("--normal-radius", type=float, default=None, metavar="R",
                    help="point_to_plane, generalized: the radius the normals are estimated with (at most 30 neighbours)")
    a = ap.parse_args()
    if a.icp_estimation != "point_to_point" and (a.icp is None or a.normal_radius is None):
        ap.error(f"--icp-estimation {a.icp_estimation} needs --icp DIST and --normal-radius R")
    if a.icp_estimation == "point_to_point" and a.normal_radius is not None:
        ap.error("--normal-radius belongs to --icp-estimation point_to_plane or generalized")

    files = sorted((f for f in os.listdir(a.source_path) if f.endswith(".pth")), key=natural_key)
    records = [torch.load(os.path.join(a.source_path, f)) for f in files]
    scenes = sorted(os.listdir(a.gt_folder))
    keys = [BM.read_trajectory(os.path.join(a.gt_folder, s, "gt.log"))[0] for s in scenes]
    if sum(len(k) for k in keys) != len(records):
        raise SystemExit(f"{len(records)} records for {sum(len(k) for k in keys)} gt pairs in {a.gt_folder}")
    summary = {}
    sampling = dict(sampler=a.sampler, sample_seeds=[(a.seed + b) % (1 << 23) for b in range(len(records))])
    if a.icp is not None:
        sampling["refine"] = a.icp
        if a.icp_estimation != "point_to_point":
            sampling.update(icp_estimation=a.icp_estimation, normal_radius=a.normal_radius)
    for n_points in a.n_points:
        np.random.seed(a.seed)
        if a.inlier_ratio:
            poses, inliers = tester.evaluate_records(records, n_points=n_points, distance_threshold=a.distance_threshold,
                                                     ransac_n=a.ransac_n, inlier_thresholds=(a.inlier_distance,),
                                                     **sampling)
        else:
            poses = tester.register_records(records, n_points=n_points, distance_threshold=a.distance_threshold,
                                            ransac_n=a.ransac_n, **sampling)
        out_dir = os.path.join(a.exp_dir, str(n_points))
        o = 0
        for scene, k in zip(scenes, keys):
            BM.write_est_trajectory(out_dir, scene, k, np.stack(poses[o:o + len(k)]))
            o += len(k)
        res = BM.benchmark(out_dir, a.gt_folder)
        summary[n_points] = {"mean_recall": res["mean_recall"], "mean_precision": res["mean_precision"]}
        if a.inlier_ratio:
            split = BM.get_scene_split(a.gt_folder)
            with open(os.path.join(out_dir, "result"), "a") as f:
                for key, label in (("wo", ""), ("w", " (mutual)")):
                    fm = BM.feature_match_recall(getattr(inliers, key)[:, 0], split, a.fmr_threshold)
                    f.write("Inlier ratio{}: {:.3f}: +- {:.3f}\n".format(label, fm["ir_mean"], fm["ir_std"]))
                    f.write("Feature match recall{}: {:.3f}: +- {:.3f}\n".format(label, fm["fmr_mean"], fm["fmr_std"]))
                    summary[n_points][f"inlier_ratio_{key}"] = fm["ir_mean"]
                    summary[n_points][f"feature_match_recall_{key}"] = fm["fmr_mean"]
        print(n_points, open(os.path.join(out_dir, "result")).read(), sep="\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
