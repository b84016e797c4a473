"""Fast global registration (registration.fast_global_registration_batch) beside RANSAC (registration.register_batch) on one
GPU: prints ONE JSON line.  Device events around the whole Python call, inputs already on the device, one warm-up, median
[min, max] of --reps calls, the two methods alternating in the same process.

  inputs : B = 64 pairs of 5 000 / 5 000 points -- bench_fpfh's bumpy surface under a random pose with 1 mm noise, described by
           its 33-wide FPFH rows (computed once, outside the timed region), and tests/ransac_ref.py's shell pairs with 32-wide
           unit descriptors (half of the source descriptors replaced by random ones); one 120 000 / 120 000 slab pair with
           32-wide unit descriptors.
  timed  : "fgr"      -- descriptors to poses: mutual L2 matching + pcrcg_fgr_batch + the one read;
           "ransac"   -- register_batch on the same inputs (50 000 hypotheses, 1 000 validations): the yardstick;
           "match"    -- mutual_match_batch alone, and "fgr_on_list" -- fast_global_registration_batch on that list
                         (correspondences=): how fgr's time splits between matching and the registration kernel.
  errors : rotation (degrees) and translation (metres) against the planted pose, the worst pair and the median, for both.

There is no earlier FGR here and no open3d timing for these inputs: RANSAC on the same inputs is the only yardstick."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import registration as REG  # noqa: E402
from scripts.bench_fpfh import bumpy_pair  # noqa: E402
from tests import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)

DELTA = 0.05


def timed_pair(fa, fb, reps):
    """Two calls timed in turn (a, b, a, b, ...) after one warm-up of each -> their two summaries."""
    fa()
    fb()
    out = ([], [])
    for _ in range(reps):
        for fn, acc in ((fa, out[0]), (fb, out[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return [{"median_ms": round(float(np.median(x)), 3), "min_ms": round(min(x), 3), "max_ms": round(max(x), 3)} for x in out]


def errors(mats, poses):
    e = np.array([RR.pose_error(T, G) for T, G in zip(mats, poses)])
    return {"rot_deg_max": float(f"{e[:, 0].max():.4g}"), "rot_deg_median": float(f"{np.median(e[:, 0]):.4g}"),
            "trans_m_max": float(f"{e[:, 1].max():.4g}"), "trans_m_median": float(f"{np.median(e[:, 1]):.4g}")}


def setting(src, tgt, fs, ft, poses, reps, delta=DELTA):
    B = len(src)
    seeds = list(range(B))
    fgr = lambda: REG.fast_global_registration_batch(src, tgt, fs, ft, maximum_correspondence_distance=delta, seeds=seeds)
    ransac = lambda: REG.register_batch(src, tgt, fs, ft, distance_threshold=delta, seeds=seeds)
    out = {"pairs": B, "points": int(src[0].shape[0]), "width": int(fs[0].shape[1]), "delta": delta}
    out["fgr"], out["ransac"] = timed_pair(fgr, ransac, reps)
    corr, k = REG.mutual_match_batch(fs, ft)
    ks = k.cpu().numpy()
    lists = [c[:kb] for c, kb in zip(corr.split([int(x.shape[0]) for x in src]), ks)]
    on_list = lambda: REG.fast_global_registration_batch(src, tgt, correspondences=lists, maximum_correspondence_distance=delta,
                                                         seeds=seeds)
    out["match"], out["fgr_on_list"] = timed_pair(lambda: REG.mutual_match_batch(fs, ft), on_list, reps)
    res = fgr()
    out["mutual_k_mean"] = round(float(ks.mean()), 1)
    out["fgr_tuples_mean"] = round(float(res.tuples.mean()), 1)
    out["fgr_trials_mean"] = round(float(res.trials.mean()), 1)
    out["fgr_errors"] = errors(res.matrices, poses)
    out["ransac_errors"] = errors(ransac().matrices, poses)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--big-n", type=int, default=120000, help="0: skip the single large pair")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    up = lambda xs: [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]
    out = {"metric": "fgr", "device": torch.cuda.get_device_name(0), "reps": a.reps}

    pairs = [bumpy_pair(100 + b, a.n) for b in range(a.batch)]
    src, tgt = up([p[0] for p in pairs]), up([p[1] for p in pairs])
    fs, ft = [], []
    for b in range(0, a.batch, 16):
        views = np.concatenate([p[3] for p in pairs[b:b + 16]])
        clouds = [x for s, t in zip(src[b:b + 16], tgt[b:b + 16]) for x in (s, t)]
        f = REG.compute_fpfh_feature_batch(clouds, 0.3, 100, normal_radius=0.15, viewpoints=views)
        fs += f[0::2]
        ft += f[1::2]
    out[f"fpfh33_{a.batch}x{a.n}"] = setting(src, tgt, fs, ft, [p[2] for p in pairs], a.reps)

    pairs = [RR.registration_pair(2000 + b, n=a.n, outliers=0.5, c=32) for b in range(a.batch)]
    out[f"unit32_{a.batch}x{a.n}"] = setting(up([p[0] for p in pairs]), up([p[1] for p in pairs]), up([p[2] for p in pairs]),
                                             up([p[3] for p in pairs]), [p[4] for p in pairs], a.reps)
    if a.big_n:
        p = RR.registration_pair(77, n=a.big_n, outliers=0.5, c=32, shape="slab")
        out[f"unit32_1x{a.big_n}"] = setting(up([p[0]]), up([p[1]]), up([p[2]]), up([p[3]]), [p[4]], a.reps, delta=0.2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
