"""Registration back end throughput on one GPU (pcrcg_amd/registration.py): prints ONE JSON line.

Settings (50 000 iterations, 1 000 validations, 32-wide descriptors, 50 % outlier descriptors):
  3dmatch  5 000 / 5 000 points on 2 m cube faces, ransac_n = 3, threshold 0.05, both checkers (ref:lib/tester.py sampling)
  kitti    5 000 / 5 000 points on a 40 m x 40 m x 0.6 m slab, ransac_n = 4, threshold 0.3
  s30k     30 000 / 30 000 points (a pair without the sampling step), ransac_n = 3, threshold 0.05
Per setting: pairs/s of `register` (matching + RANSAC + its one read-back, median of --reps) and the median ms of the
stages from events: nn (pcrcg_feature_match), hypotheses (pcrcg_ransac with max_validation = 1: draws, checks, fits,
compaction, one evaluation, selection) and evaluation (pcrcg_ransac at 1 000 validations minus that).

  sampling (--settings sampling)  the stage before registration: 64 pairs of 2 x 20 000 points -> 5 000 interest points
           per cloud on overlap x saliency.  device: tester.probabilistic_sample_batch (registration.sample_batch + gather)
           on inputs that are on the device, between events, after a warm-up, median of --reps; host:
           tester._sample_records on the same records as CPU tensors (what the evaluation scripts hand it), wall clock,
           median of --reps (at most 5)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from pcrcg_amd import registration as REG  # noqa: E402
import ransac_ref as RR  # noqa: E402   (the synthetic pair generator)

SETTINGS = {
    "3dmatch": dict(n=5000, shape="shell", ransac_n=3, thr=0.05, noise=0.003),
    "kitti": dict(n=5000, shape="slab", ransac_n=4, thr=0.3, noise=0.005),
    "s30k": dict(n=30000, shape="shell", ransac_n=3, thr=0.05, noise=0.003),
}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def bench(name, s, reps, max_iteration, max_validation):
    dev = torch.device("cuda:0")
    src, tgt, f, g, T_gt = RR.registration_pair(1, n=s["n"], outliers=0.5, noise=s["noise"], shape=s["shape"])
    src, tgt, f, g = (torch.from_numpy(x).to(dev) for x in (src, tgt, f, g))
    kw = dict(distance_threshold=s["thr"], ransac_n=s["ransac_n"], max_iteration=max_iteration, seed=0)
    res = REG.register(src, tgt, f, g, max_validation=max_validation, **kw)           # warm-up + accuracy
    rot, trans = RR.pose_error(res.matrix, T_gt)
    total = timed(lambda: REG.register(src, tgt, f, g, max_validation=max_validation, **kw), reps)
    nn = timed(lambda: REG.feature_match(f, g), reps)
    hyp = timed(lambda: REG.register(src, tgt, f, g, max_validation=1, **kw), reps) - nn
    full = total - nn
    return {"pairs_per_s": round(1000.0 / total, 2), "ms_total": round(total, 3), "ms_nn": round(nn, 3),
            "ms_hypotheses": round(hyp, 3), "ms_evaluation": round(full - hyp, 3), "validations": res.validations,
            "fitness": round(res.fitness, 4), "rot_err_deg": round(rot, 4), "trans_err": round(trans, 5)}


def bench_sampling(reps, pairs=64, n=20000, keep=5000, c=32):
    import time
    from pcrcg_amd import tester
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    records = [{"pcd": torch.from_numpy(rng.rand(2 * n, 3).astype(np.float32)),
                "feats": torch.from_numpy(rng.randn(2 * n, c).astype(np.float32)),
                "overlaps": torch.from_numpy(rng.rand(2 * n).astype(np.float32)),
                "saliency": torch.from_numpy(rng.rand(2 * n).astype(np.float32)), "len_src": n} for _ in range(pairs)]
    pcds, feats, scores = [], [], []
    for r in records:
        sc = (r["overlaps"] * r["saliency"]).to(dev)
        p, f = r["pcd"].to(dev), r["feats"].to(dev)
        pcds += [p[:n], p[n:]]
        feats += [f[:n], f[n:]]
        scores += [sc[:n], sc[n:]]
    seeds = list(range(2 * pairs))
    run = lambda: tester.probabilistic_sample_batch(pcds, feats, scores, keep, seeds)
    run()                                                                            # warm-up
    torch.cuda.synchronize()
    device_ms = timed(run, reps)
    select_ms = timed(lambda: REG.sample_batch(scores, keep, seeds), reps)
    host = []
    np.random.seed(0)
    for _ in range(min(reps, 5)):
        t0 = time.perf_counter()
        tester._sample_records(records, keep)
        host.append(1e3 * (time.perf_counter() - t0))
    host_ms = float(np.median(host))
    return {"pairs": pairs, "points": n, "keep": keep, "device_ms": round(device_ms, 3),
            "device_select_ms": round(select_ms, 3), "device_ms_per_pair": round(device_ms / pairs, 4),
            "host_ms": round(host_ms, 2), "host_ms_per_pair": round(host_ms / pairs, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settings", default="3dmatch,kitti,s30k")
    ap.add_argument("--max-iteration", type=int, default=50000)
    ap.add_argument("--max-validation", type=int, default=1000)
    a = ap.parse_args()
    out = {"metric": "registration", "max_iteration": a.max_iteration, "max_validation": a.max_validation,
           "device": torch.cuda.get_device_name(0)}
    for name in a.settings.split(","):
        if name == "sampling":
            out[name] = bench_sampling(a.reps)
            continue
        out[name] = bench(name, SETTINGS[name], a.reps, a.max_iteration, a.max_validation)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
