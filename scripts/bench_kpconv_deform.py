"""Time a deformable, modulated KPConv layer of S30k geometry on one MI355X.

Levels 2 and 3 of the S30k synthetic pair with the tables a deformable layer gets (built at deform_radius), cin = cout =
256 and 512 as the indoor architecture has there.  Per level, three comparisons:

  module   blocks.KPConv(deformable, modulated): offset convolution + bias, general gather (kpconv_ex), contraction
  dense    the reference's dense formulation (ref:models/blocks.py:229-374) restated in torch on the same GPU
  rigid    ops.kpconv_ex in rigid / linear / sum mode against ops.kpconv on the same inputs: the price of the general
           kernel where the specialised one applies

HIP event pairs around CALLS back-to-back calls, no read-back inside a window, the configurations alternating inside
each of REPEATS repeats after a warm-up; median and [min, max] over the repeats.  Prints one JSON line per level."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcrcg_amd import indoor_config, ops, synthetic  # noqa: E402
from pcrcg_amd.blocks import KPConv  # noqa: E402
from pcrcg_amd.pyramid import build_pyramid  # noqa: E402

LIMITS = [43, 42, 47, 43]       # tests/golden/calibration.json, S30k


def dense_kpconv(q_pts, s_pts, inds, x, kernel_points, weights, extent, off=None):
    """One KPConv of the reference's formulation with torch tensors: [nq, H, K] distances, for a deformed kernel the kept
    columns compacted with topk, a batched matmul per stage.  -> out, share of the real neighbours out of range."""
    K = kernel_points.shape[0]
    s_pad = torch.cat((s_pts, torch.zeros_like(s_pts[:1]) + 1e6), 0)
    nb = s_pad[inds] - q_pts.unsqueeze(1)
    kp_q = kernel_points if off is None else (off[:, :3 * K].view(-1, K, 3) * extent + kernel_points).unsqueeze(1)
    d2 = ((nb.unsqueeze(2) - kp_q) ** 2).sum(3)
    skipped = 0.0
    if off is not None:
        in_range = (d2 < extent ** 2).any(2).to(torch.int32)
        flag, cols = torch.topk(in_range, int(in_range.sum(1).max()), dim=1)
        inds = inds.gather(1, cols) * flag - (flag.to(torch.int64) - 1) * int(s_pad.shape[0] - 1)
        d2 = d2.gather(1, cols.unsqueeze(2).expand(-1, -1, K))
        skipped = float(1.0 - in_range.sum() / max(int((nb[..., 0] < 1e5).sum()), 1))
    w = torch.clamp(1 - torch.sqrt(d2) / extent, min=0.0).transpose(1, 2)
    nx = torch.cat((x, torch.zeros_like(x[:1])), 0)[inds]
    wf = torch.matmul(w, nx)
    if off is not None:
        wf = wf * (2 * torch.sigmoid(off[:, 3 * K:])).unsqueeze(2)
    out = torch.matmul(wf.permute(1, 0, 2), weights).sum(0)
    n = torch.clamp((nx.sum(-1) > 0).sum(-1), min=1)
    return out / n.unsqueeze(1), skipped


def dense_reference(conv, q_pts, s_pts, inds, x):
    oc = conv.offset_conv
    off = dense_kpconv(q_pts, s_pts, inds, x, oc.kernel_points, oc.weights, oc.KP_extent)[0] + conv.offset_bias
    return dense_kpconv(q_pts, s_pts, inds, x, conv.kernel_points, conv.weights, conv.KP_extent, off)


def timed(fns, calls, repeats, warmup):
    """fns: name -> callable; -> name -> [median, min, max] microseconds per call."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for name, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / calls)
    return {k: [round(float(np.median(v)), 1), round(min(v), 1), round(max(v), 1)] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kpconv_deform.py needs a HIP device")
    dev = torch.device("cuda:0")
    cfg = indoor_config(modulated=True)
    cfg["architecture"][6:11] = ["resnetb_deformable", "resnetb_deformable", "resnetb_deformable_strided",
                                 "resnetb_deformable", "resnetb_deformable"]
    src, tgt = synthetic.pair("S30k", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(dev)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=dev)
    batch = build_pyramid(pts, lens, cfg, LIMITS)
    for level, cin in ((2, 256), (3, 512)):
        q = s = batch["points"][level]
        inds = batch["neighbors"][level]
        r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** level
        torch.manual_seed(level)
        np.random.seed(level)
        conv = KPConv(15, 3, cin, cin, r * cfg.KP_extent / cfg.conv_radius, r, deformable=True, modulated=True).to(dev)
        x = torch.randn(s.shape[0], cin, device=dev)
        with torch.no_grad():
            conv.weights.normal_(0, 0.05)
            conv.offset_bias.normal_(0, 0.08)
            raw = conv.offset_conv(q, s, inds, x)
            conv.offset_conv.weights.mul_(0.08 / float(raw[:, :45].pow(2).mean().sqrt()))    # rms offset ~0.11 of the extent
            ours = conv(q, s, inds, x)
            ref, skipped = dense_reference(conv, q, s, inds, x)
            kp, w = conv.kernel_points.data, conv.weights.data
            fns = {"module": lambda: conv(q, s, inds, x),
                   "dense_torch": lambda: dense_reference(conv, q, s, inds, x),
                   "offset_conv": lambda: conv.offset_conv(q, s, inds, x),
                   "kpconv_ex_deformed": lambda: ops.kpconv_ex(q, s, inds, x, kp, w, conv.KP_extent,
                                                               offset_features=conv.offset_features, modulated=True,
                                                               want_min_d2=True),
                   "kpconv_ex_rigid": lambda: ops.kpconv_ex(q, s, inds, x, kp, w, conv.KP_extent),
                   "kpconv_rigid": lambda: ops.kpconv(q, s, inds, x, kp, w, conv.KP_extent)}
            t = timed(fns, args.calls, args.repeats, args.warmup)
            price = float((ops.kpconv_ex(q, s, inds, x, kp, w, conv.KP_extent) - ops.kpconv(q, s, inds, x, kp, w, conv.KP_extent))
                          .abs().max() / ref.abs().max())
        # rows within 1e-4 (relative, of max|ref|) of the dense formulation: the others sit at a kept-set threshold
        close = float(((ours - ref).abs().amax(1) <= 1e-4 * ref.abs().max()).float().mean())
        print(json.dumps(dict(level=level, rows=int(q.shape[0]), H=int(inds.shape[1]), cin=cin, cout=cin,
                              real_neighbours_skipped=round(skipped, 4), rows_within_1e4_of_dense=round(close, 4),
                              rigid_ex_vs_kpconv_max_dev=price, us_per_call_median_min_max=t)), flush=True)


if __name__ == "__main__":
    main()
