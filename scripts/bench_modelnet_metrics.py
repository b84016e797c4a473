"""The modified Chamfer distance of the ModelNet test set's size on one GPU; prints ONE JSON line.

1 266 pairs (the ModelNet40 test split of the reference) of 717 / 717 / 2048 points (--distinct synthetic pairs of
pcrcg_amd.synthetic.modelnet_pairs, reused cyclically; predictions = ground truth moved by a small residual), all
inputs already on the device.  Device events around each timed call, --warmup calls first, the median of --reps:
  (a) batched_ms   one modelnet.chamfer_batch call over all pairs, its one read-back included;
  (b) torch_gpu_ms the reference's formulation in torch on the same GPU, pair by pair as its tester runs it (two dense
                   [n, m] squared-distance matrices and torch.min per pair; written out here from the formula);
  (c) torch_cpu_ms the same in torch on the CPU (--cpu-threads threads) for --cpu-pairs pairs, scaled to all pairs.
glanes: 2 n m candidate-query evaluations per pair over (a), in 1e9 per second.  check: the largest relative difference
between (a)'s and (b)'s chamfer values."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import modelnet, synthetic  # noqa: E402


def torch_pair(src, ref, raw, P, G):
    """compute_metrics' modified Chamfer distance of one pair (batch of one), dense, in the tensors' device and fp32."""
    def inv(g):
        r, t = g[:, :3, :3], g[:, :3, 3]
        return torch.cat([r.transpose(-1, -2), r.transpose(-1, -2) @ -t[..., None]], -1)

    def cat(a, b):
        return torch.cat([a[:, :3, :3] @ b[:, :3, :3], a[:, :3, :3] @ b[:, :3, 3:] + a[:, :3, 3:]], -1)

    def move(g, a):
        return a @ g[:, :3, :3].transpose(-1, -2) + g[:, :3, 3][:, None, :]

    def sq(a, b):
        return torch.sum((a[:, :, None, :] - b[:, None, :, :]) ** 2, -1)

    ds = torch.min(sq(move(P, src), raw), -1)[0]
    dr = torch.min(sq(ref, move(cat(P, inv(G)), raw)), -1)[0]
    return torch.mean(ds, 1) + torch.mean(dr, 1)


def event_timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1266)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-pairs", type=int, default=50)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--only-batched", action="store_true", help="(a) alone: the run to put under a kernel trace")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    base = synthetic.modelnet_pairs(a.distinct, 0)
    rng = np.random.RandomState(1)
    for p in base:
        pose = np.concatenate([synthetic._pose(rng, angle=0.3, shift=0.1)[:3] @ np.concatenate([p["transform_gt"], [[0, 0, 0, 1]]]),
                               [[0, 0, 0, 1]]])
        p["pred"] = pose.astype(np.float32)
    pick = [base[b % a.distinct] for b in range(a.pairs)]
    on = {k: [torch.from_numpy(p[k]).to(dev) for p in base] for k in ("points_src", "points_ref", "points_raw")}
    lists = [[on[k][b % a.distinct] for b in range(a.pairs)] for k in ("points_src", "points_ref", "points_raw")]
    pred = torch.from_numpy(np.stack([p["pred"] for p in pick])).to(dev)
    gt = torch.from_numpy(np.stack([p["transform_gt"] for p in pick])).to(dev)
    res = modelnet.chamfer_batch(*lists, pred, gt)
    n, m, r = (int(x[0]) for x in (res.n_src, res.n_ref, res.n_raw))
    out = {"pairs": a.pairs, "sizes": [n, m, r], "warmup": a.warmup, "reps": a.reps}
    med, lo, hi = event_timed(lambda: modelnet.chamfer_batch(*lists, pred, gt), a.warmup, a.reps)
    out.update(batched_ms=round(med, 3), batched_min_max_ms=[round(lo, 3), round(hi, 3)],
               glanes=round((n + m) * r * a.pairs / med / 1e6, 1), chamfer_mean=float(res.chamfer.mean()))
    if not a.only_batched:
        def loop():
            vals = [torch_pair(lists[0][b][None], lists[1][b][None], lists[2][b][None], pred[b:b + 1], gt[b:b + 1])
                    for b in range(a.pairs)]
            return torch.cat(vals).cpu()
        ref = loop().numpy()
        med, lo, hi = event_timed(loop, a.warmup, a.reps)
        out.update(torch_gpu_ms=round(med, 1), torch_gpu_min_max_ms=[round(lo, 1), round(hi, 1)],
                   speedup_vs_torch_gpu=round(med / out["batched_ms"], 1),
                   check=float(np.max(np.abs(ref - res.chamfer) / np.abs(ref))))
        torch.set_num_threads(a.cpu_threads)
        host = [[t.cpu() for t in x[:a.cpu_pairs]] for x in lists]
        hp, hg = pred.cpu(), gt.cpu()
        cpu_loop = lambda: [torch_pair(host[0][b][None], host[1][b][None], host[2][b][None], hp[b:b + 1], hg[b:b + 1])  # noqa: E731
                            for b in range(len(host[0]))]
        cpu_loop()
        t0 = time.perf_counter()
        cpu_loop()
        out.update(torch_cpu_ms=round((time.perf_counter() - t0) * 1e3 * a.pairs / len(host[0]), 1), cpu_pairs=len(host[0]),
                   cpu_threads=a.cpu_threads)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
