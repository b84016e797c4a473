"""Time forward + backward of a deformable, modulated KPConv layer of S30k geometry on one MI355X.

The tables and the protocol of scripts/bench_kpconv_deform.py: levels 2 and 3 of the S30k synthetic pair with the tables a
deformable layer gets, cin = cout = 256 and 512.  Per level, forward + backward (gradients of x, weights,
offset_conv.weights and offset_bias for an upstream dy) of

  module   train_forward._kpconv on blocks.KPConv(deformable, modulated): offset convolution (AG.kpconv) + bias,
           AG.kpconv_ex (pcrcg_kpconv_aggregate_ex, pcrcg_kpconv_backward_ex, three products)
  dense    the reference's dense formulation (ref:models/blocks.py:229-374) restated in torch, under torch autograd, on
           the same GPU
  rigid    AG.kpconv forward + backward on the same inputs: the price of a rigid layer
  ex_only  AG.kpconv_ex alone with the module's offset_features as a leaf (the new operator without the offset convolution)

HIP event pairs around CALLS back-to-back calls, no read-back inside a window, the configurations alternating inside
each of REPEATS repeats after a warm-up; median and [min, max] over the repeats.  Prints one JSON line per level."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_kpconv_deform import LIMITS, dense_reference, timed  # noqa: E402
from pcrcg_amd import autograd as AG  # noqa: E402
from pcrcg_amd import indoor_config, synthetic, train_forward  # noqa: E402
from pcrcg_amd.blocks import KPConv  # noqa: E402
from pcrcg_amd.pyramid import build_pyramid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kpconv_deform_train.py needs a HIP device")
    dev = torch.device("cuda:0")
    cfg = indoor_config(modulated=True)
    src, tgt = synthetic.pair("S30k", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(dev)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=dev)
    cfg["architecture"][6:11] = ["resnetb_deformable", "resnetb_deformable", "resnetb_deformable_strided",
                                 "resnetb_deformable", "resnetb_deformable"]
    batch = build_pyramid(pts, lens, cfg, LIMITS)
    for level, cin in ((2, 256), (3, 512)):
        q = s = batch["points"][level]
        inds = batch["neighbors"][level]
        r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** level
        torch.manual_seed(level)
        np.random.seed(level)
        conv = KPConv(15, 3, cin, cin, r * cfg.KP_extent / cfg.conv_radius, r, deformable=True, modulated=True).to(dev)
        x = torch.randn(s.shape[0], cin, device=dev).requires_grad_(True)
        dy = torch.randn(q.shape[0], cin, device=dev)
        with torch.no_grad():
            conv.weights.normal_(0, 0.05)
            conv.offset_bias.normal_(0, 0.08)
            raw = conv.offset_conv(q, s, inds, x)
            conv.offset_conv.weights.mul_(0.08 / float(raw[:, :45].pow(2).mean().sqrt()))    # rms offset ~0.11 of the extent
        params = [x, conv.weights, conv.offset_conv.weights, conv.offset_bias]
        kp = conv.kernel_points.data

        def clear():
            for p in params:
                p.grad = None

        def module():
            clear()
            train_forward._kpconv(conv, q, s, inds, x).backward(dy)

        def dense():
            clear()
            dense_reference(conv, q, s, inds, x)[0].backward(dy)

        def rigid():
            clear()
            AG.kpconv(x, conv.weights, q, s, inds, kp, conv.KP_extent).backward(dy)

        module()
        off = conv.offset_features.clone().requires_grad_(True)
        ours = {k: p.grad.clone() for k, p in zip(("x", "weights", "offset_weights", "offset_bias"), params)}

        def ex_only():
            clear()
            off.grad = None
            AG.kpconv_ex(x, conv.weights, q, s, inds, kp, conv.KP_extent, offset_features=off, modulated=True)[0].backward(dy)

        dense()
        dev_rel = {k: float((ours[k] - p.grad).abs().max() / p.grad.abs().max())
                   for k, p in zip(("x", "weights", "offset_weights", "offset_bias"), params)}
        t = timed({"module": module, "dense_torch": dense, "rigid_kpconv": rigid, "kpconv_ex_only": ex_only},
                  args.calls, args.repeats, args.warmup)
        print(json.dumps(dict(level=level, rows=int(q.shape[0]), H=int(inds.shape[1]), cin=cin, cout=cin,
                              max_dev_from_dense_all_rows=dev_rel, fwd_bwd_us_per_call_median_min_max=t)), flush=True)


if __name__ == "__main__":
    main()
