"""Inlier ratios of the 3DMatch test set's size on one GPU: registration.inlier_ratio_batch (every pair in one batched
call) against the per-pair registration.get_inlier_ratio loop; prints ONE JSON line.

1 623 pairs (the 3DMatch test set) of --points / --points points with 32-wide descriptors (the --distinct synthetic pairs
of tests/ransac_ref.py, 50 % outlier descriptors, reused cyclically), all inputs already on the device, the 20 distance
thresholds of benchmark.fmr_wrt_distance.  batched_s: the median of --reps timed calls, each including its one read-back;
loop_s: one pass of get_inlier_ratio over the same pairs (threshold 0.1).  gflops: both arg-max directions,
2 x 2 n m C per pair, over batched_s."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from pcrcg_amd import benchmark as BM  # noqa: E402
from pcrcg_amd import registration as REG  # noqa: E402
import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1623)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true", help="skip the per-pair loop")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    base = []
    for b in range(a.distinct):
        src, tgt, f, g, T = RR.registration_pair(900 + b, n=a.points, outliers=0.5)
        base.append([torch.from_numpy(x).to(dev) for x in (src, tgt, f, g)] + [T[:3, :3], T[:3, 3]])
    pairs = [base[b % a.distinct] for b in range(a.pairs)]
    lists = [list(x) for x in zip(*pairs)]
    run = lambda: REG.inlier_ratio_batch(*lists, thresholds=BM.FMR_DISTANCES)   # noqa: E731
    res = run()                                                                   # warm-up (and the library load)
    batched = timed(run, a.reps)
    out = {"pairs": a.pairs, "points": a.points, "c": 32, "thresholds": len(BM.FMR_DISTANCES),
           "batched_s": round(batched, 4),
           "gflops": round(4.0 * a.points * a.points * 32 * a.pairs / batched / 1e9, 1),
           "ir_wo_mean": round(float(res.wo[:, 9].mean()), 4), "ir_w_mean": round(float(res.w[:, 9].mean()), 4)}
    if not a.no_loop:
        REG.get_inlier_ratio(*pairs[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = [REG.get_inlier_ratio(*p) for p in pairs]
        torch.cuda.synchronize()
        out["loop_s"] = round(time.perf_counter() - t0, 3)
        out["speedup"] = round(out["loop_s"] / batched, 1)
        out["loop_ir_wo_mean"] = round(float(np.mean([float(r["wo"]["inlier_ratio"]) for r in ref])), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
