"""Preparing the ModelNet test split's pairs on one GPU (pcrcg_amd/modelnet_prep.py): prints ONE JSON line.

Workload: the shape of the 1 266-pair test split -- [2048, 6] clouds (synthetic.modelnet_clouds) through the `crop` test
chain of modelnet_config() (partial [0.7, 0.7], 717 / 717 rows out) -- in ONE prepare_pairs call, inputs already on the
device.  Every timed call ends with a device synchronise; the median of --reps calls after one warm-up:

  transform_ms : transform_pairs -- the host's draws, one crop call, one read-back, one assemble call
  prepare_ms   : prepare_pairs   -- the same plus ONE get_correspondences_batch call and the item dicts
  draws_ms     : the host's draws alone (modelnet_prep.draws over the pairs; part of both figures above and of numpy_ms)
  numpy_ms     : the numpy restatement of the same chains (tests/modelnet_prep_ref.py run_chain under the same draws) pair by
                 pair on this host's CPU -- the transforms only, no correspondences (the reference finds those with open3d)

Before anything is timed the device's reference-side clouds are compared with the restatement's bit for bit on the first
--check pairs.  Nothing printed is a speed-up over the reference's loader, which needs open3d and torchvision: it is not timed.
Recorded on one MI355X (one run, medians as above, spread not measured): transform_ms 256.76,
prepare_ms 327.04, draws_ms 158.08, numpy_ms 545.17 on that host's CPU; one crop call, one assemble call, one
correspondence call, one read-back; 693 correspondences per pair on average."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import modelnet_config, synthetic  # noqa: E402
from pcrcg_amd import modelnet_prep as MP  # noqa: E402
from tests import modelnet_prep_ref as PR  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=1266)
    ap.add_argument("--check", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = modelnet_config()
    B = a.pairs
    clouds = synthetic.modelnet_clouds(B, 5)
    labels = np.arange(B) % 40
    idxs = list(range(B))
    steps = MP.get_transforms(cfg.noise_type, cfg.rot_mag, cfg.trans_mag, cfg.num_points, cfg.partial)[1]
    on_dev = torch.from_numpy(clouds).to(dev)
    rng = np.random.RandomState(0)

    before = dict(MP.CALLS)
    items = MP.prepare_pairs(on_dev, labels, idxs, cfg, rng=rng)                         # warm-up, the counts, the comparison
    calls = {k: MP.CALLS[k] - before[k] for k in before}
    same = True
    for b in range(min(a.check, B)):
        kept = [int(items[b]["sample"]["points_" + s].shape[1]) for s in ("src", "ref")]
        d = MP.draws(2048, b, steps, rng)
        want, _ = PR.run_chain(clouds[b], b, steps, d)
        same &= kept == [717, 717] and want["points_ref"].tobytes() == items[b]["sample"]["points_ref"][0].cpu().numpy().tobytes()

    def numpy_side():
        for b in range(B):
            d = MP.draws(2048, b, steps, rng)
            PR.run_chain(clouds[b], b, steps, d)

    out = {"metric": "modelnet_prep", "device": torch.cuda.get_device_name(0), "reps": a.reps, "pairs": B, "rows_in": 2048,
           "rows_out": [717, 717], "library_calls": {"crop": calls["crop"], "assemble": calls["assemble"], "correspondences": 1},
           "read_backs_of_kept_counts": calls["read_back"], "reference_side_bit_identical_to_numpy": bool(same),
           "n_correspondences_mean": float(np.mean([it["n_correspondences"] for it in items]))}
    out["transform_ms"] = round(1e3 * timed(lambda: MP.transform_pairs(on_dev, idxs, steps, rng, labels=labels), a.reps, True), 2)
    out["prepare_ms"] = round(1e3 * timed(lambda: MP.prepare_pairs(on_dev, labels, idxs, cfg, rng=rng), a.reps, True), 2)
    out["draws_ms"] = round(1e3 * timed(lambda: [MP.draws(2048, b, steps, rng) for b in range(B)], min(a.reps, 3), False), 2)
    out["numpy_ms"] = round(1e3 * timed(numpy_side, min(a.reps, 3), False), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
