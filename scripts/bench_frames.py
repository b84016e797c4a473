"""Raw frames against precomputed projections for PCR-CG's image branch (img_num 2, S30k pairs): prints ONE JSON line.

1. GPU time per pair of the input build, CUDA events over --reps repetitions: pcrcg_inject_frames (4 frames, projection
   included, one launch) against pcrcg_fill2d + 4 x pcrcg_inject_image_features fed resident projections, and against
   the whole unfused device path (4 x pcrcg_project_depth + fill + 4 injections).
2. Engine pairs/s on the S30k_img129 leg at bench.py's settings (3 model streams, 1 front thread, 4 pairs per build and per
   forward, 96 pairs per region after 8 of warm-up) with raw frames against precomputed projections: --regions
   interleaved regions of each, median and spread.
3. Host cost of the same projection arithmetic in torch on the CPU (4 projections per pair) with 1 and 16 threads, for
   comparison: what a loader that projects pays per pair."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import indoor_config, ops, synthetic  # noqa: E402
from pcrcg_amd.architectures import KPFCNN  # noqa: E402
from pcrcg_amd.projection import Projection, superglue_valid_maps  # noqa: E402


def pair_inputs(seed, dev, net):
    """(points (pinned host), lengths (pinned host), frame images, projection images) of S30k pair `seed`."""
    src, tgt = synthetic.pair("S30k", seed)
    fr = synthetic.frame_inputs(src, tgt, seed, img_num=2)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(dev)
    batch = {"points": [pts], "src_pcd_raw": pts[:len(src)]}
    for k, v in fr.items():
        if not k.startswith("sg"):
            t = torch.from_numpy(v)
            batch[k] = t if k.endswith(("_world2camera", "_intrinsics")) else t.to(dev)
    for i in (1, 2):
        s, t = superglue_valid_maps(*(torch.from_numpy(fr[f"sg{i}_{k}"]).to(dev)
                                      for k in ("keypoints0", "keypoints1", "matches", "confidence")))
        batch[f"src_valid_map{i}"], batch[f"tgt_valid_map{i}"] = s, t
    proj = {k: v for k, v in batch.items() if not k.endswith(("_depth", "_world2camera", "_intrinsics"))}
    for side, cloud in (("src", pts[:len(src)]), ("tgt", pts[len(src):])):
        for i in (1, 2):
            proj[f"{side}{i}_inds2d"], proj[f"{side}{i}_inds3d"] = Projection(batch[f"{side}{i}_intrinsics"]).projection(
                cloud, batch[f"{side}{i}_depth"], batch[f"{side}{i}_world2camera"])
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32)
    return (pts.cpu().pin_memory(), lens.pin_memory(), net.image_list(batch)[2], net.image_list(proj)[2], batch, len(src))


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernel_times(dev, inp, reps):
    hp, _, frames, projs, batch, len_src = inp
    pts = hp.to(dev)
    n = int(pts.shape[0])
    f = lambda: ops.inject_frames(pts, len_src, frames, width=132)  # noqa: E731
    p = lambda: ops.inject_image_features(n, len_src, projs, width=132)  # noqa: E731

    def unfused():
        ims = []
        for im, fr in zip(projs, frames):
            cloud = pts[len_src:] if fr["target"] else pts[:len_src]
            i2, i3 = Projection(fr["intrinsics"]).projection(cloud, fr["depth"], fr["world2camera"])
            ims.append(dict(im, inds2d=i2, inds3d=i3))
        return ops.inject_image_features(n, len_src, ims, width=132)
    x = f()
    assert torch.equal(x, p())
    return {"inject_frames_us": round(1e3 * event_ms(f, reps), 2),
            "fill2d_plus_4_inject_image_features_us": round(1e3 * event_ms(p, reps), 2),
            "4_project_depth_plus_fill_plus_4_inject_us (count read back per projection)": round(1e3 * event_ms(unfused, max(reps // 10, 5)), 2),
            "points": n, "rows_with_image_features": int((x[:, :128] != 1).any(1).sum()), "reps": reps}


def engine(dev, net, cfg, pool, kind, workers=3, ppf=4, ppb=4):
    from pcrcg_amd.pairstream import PairStreams
    pipe = PairStreams(net, cfg, synthetic.LIMITS["S30k"], dev, model_streams=workers, front_threads=1, up_nearest=False,
                       pairs_per_forward=ppf, pairs_per_build=ppb)

    def run(count):
        sub = 0
        for i in range(count):
            while sub < min(count, i + 6 * ppb):
                hp, hl, frames, projs = pool[sub % len(pool)][:4]
                pipe.submit(hp.to(dev, non_blocking=True), hl.to(dev, non_blocking=True),
                            images=frames if kind == "frames" else projs)
                sub += 1
            pipe.result(wait=False)
    run(3 * workers * ppf)
    pipe.drain()
    return pipe, run


def cpu_projection_ms(inp, threads, reps=5):
    """The reference's projection arithmetic in torch on the CPU, 4 projections (one pair at img_num 2)."""
    hp, _, frames, _, _, len_src = inp
    torch.set_num_threads(threads)
    items = []
    for fr in frames:
        cloud = (hp[len_src:] if fr["target"] else hp[:len_src]).clone()
        K = torch.eye(4)
        K[:3, :3] = torch.as_tensor(fr["intrinsics"])
        items.append((cloud, fr["depth"].cpu(), torch.as_tensor(fr["world2camera"]).float(), K))

    def one(points, depth, w2c, K):
        ones = torch.ones((1, points.shape[0]))
        cam = torch.mm(w2c, torch.cat([points.t(), ones])).t()[:, :3]
        img = torch.mm(K, torch.cat([cam.t(), ones])).t()[:, :3]
        z = img[:, 2]
        xy = (img[:, :2] / z.repeat(2, 1).T).long()
        m = (xy[:, 1] >= 0) & (xy[:, 1] < depth.shape[0]) & (xy[:, 0] >= 0) & (xy[:, 0] < depth.shape[1])
        d = depth[xy[m, 1], xy[m, 0]]
        md = torch.abs(z[m] - d) < 0.1
        return xy[m][md], torch.arange(points.shape[0])[m][md]
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for it in items:
            one(*it)
        out.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(out)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=4)
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--skip-engine", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = indoor_config(image_feature=True, img_num=2, in_feats_dim=129)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).eval().to(dev)
    with torch.no_grad():
        pool = [pair_inputs(s, dev, net) for s in range(4)]
        rec = {"kernels_per_pair": kernel_times(dev, pool[0], args.reps)}
        if not args.skip_engine:
            engines = {k: engine(dev, net, cfg, pool, k) for k in ("projections", "frames")}
            rates = {k: [] for k in engines}
            for _ in range(args.regions):
                for k, (pipe, run) in engines.items():
                    run(args.warmup)
                    pipe.drain()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(args.steps)
                    pipe.drain()
                    torch.cuda.synchronize()
                    rates[k].append(args.steps / (time.perf_counter() - t0))
            for pipe, _ in engines.values():
                pipe.close()
            rec["engine_S30k_img129_pairs_per_s"] = {
                k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                    "regions": [round(r, 1) for r in v]} for k, v in rates.items()}
    rec["host_torch_projection_ms_per_pair"] = {f"{t}_threads": cpu_projection_ms(pool[0], t) for t in (1, 16)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
