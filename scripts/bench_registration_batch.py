"""Several pairs per call (registration.register_batch) against one pair per call (registration.register) on one GPU:
prints ONE JSON line.

Settings as scripts/bench_registration.py (5 000 / 5 000 points, 32-wide descriptors, 50 % outlier descriptors,
50 000 iterations, 1 000 validations): 3dmatch (ransac_n = 3, threshold 0.05, both checkers) and kitti (ransac_n = 4,
threshold 0.3).  Per setting: pairs/s of `register` and of `register_batch` at B = 1, 16, 64, 256 (the median of --reps
timed calls, each including its one read-back), from the same process and the same pairs.  Then the wall time of one
full-size pass: 1 623 pairs (the 3DMatch test set) at 5 000 points, the distinct synthetic pairs reused cyclically, all
inputs already on the device."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from pcrcg_amd import registration as REG  # noqa: E402
import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)

SETTINGS = {
    "3dmatch": dict(shape="shell", ransac_n=3, thr=0.05, noise=0.003),
    "kitti": dict(shape="slab", ransac_n=4, thr=0.3, noise=0.005),
}


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--settings", default="3dmatch,kitti")
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--full-pairs", type=int, default=1623)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    out = {"metric": "registration_batch", "n_points": a.n, "max_iteration": 50000, "max_validation": 1000,
           "device": torch.cuda.get_device_name(0)}
    for name in a.settings.split(","):
        s = SETTINGS[name]
        pairs = []
        for b in range(max(batches)):
            src, tgt, f, g, _ = RR.registration_pair(1000 + b, n=a.n, outliers=0.5, noise=s["noise"], shape=s["shape"])
            pairs.append([torch.from_numpy(x).to(dev) for x in (src, tgt, f, g)])
        kw = dict(distance_threshold=s["thr"], ransac_n=s["ransac_n"])
        REG.register(*pairs[0], **kw)
        single = timed(lambda: REG.register(*pairs[0], **kw), a.reps * 3)
        row = {"single_pairs_per_s": round(1.0 / single, 1), "single_ms": round(1e3 * single, 3)}
        for B in batches:
            lists = [list(x) for x in zip(*pairs[:B])]
            seeds = list(range(B))
            REG.register_batch(*lists, seeds=seeds, **kw)
            t = timed(lambda: REG.register_batch(*lists, seeds=seeds, **kw), a.reps)
            row[f"B{B}"] = {"pairs_per_s": round(B / t, 1), "ms_per_call": round(1e3 * t, 3),
                            "speedup": round(single * B / t, 2)}
        out[name] = row
        if name == "3dmatch" and a.full_pairs:
            P = len(pairs)
            lists = [[pairs[i % P][j] for i in range(a.full_pairs)] for j in range(4)]
            seeds = list(range(a.full_pairs))
            res = REG.register_batch(*lists, seeds=seeds, **kw)
            t = timed(lambda: REG.register_batch(*lists, seeds=seeds, **kw), 3)
            out["full_pass"] = {"pairs": a.full_pairs, "seconds": round(t, 3), "pairs_per_s": round(a.full_pairs / t, 1),
                                "single_pair_estimate_s": round(single * a.full_pairs, 3),
                                "mean_fitness": round(float(np.mean(res.fitness)), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
