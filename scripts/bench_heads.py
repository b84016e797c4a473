"""Time KPFCNN's node-overlap and pose heads on one MI355X: S30k synthetic pair, full-width model,
op-by-op path (the C++ runners do not sequence the heads).

  forward_ops        the inference forward with and without the heads (both models on the op-by-op path)
  folding chain      the five Linear + ReLU of folding1 on the normalised feats_f [N, 32] -> h [N, 1024]
  last folding layer Linear(512, 1024) + ReLU alone: the write of h
  tail               ops.pose_head on h (linear1, linear2, normalisation, means; one read of h), and its backward; bytes over
                     time against the 8 TB/s roofline
  train              forward_train + backward of a linear functional of the outputs, with and without the heads

HIP event pairs around CALLS back-to-back calls, no read-back inside a window, the configurations alternating inside each
of REPEATS repeats after a warm-up; median and [min, max] over the repeats.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcrcg_amd import indoor_config, ops, synthetic  # noqa: E402
from pcrcg_amd.architectures import KPFCNN  # noqa: E402
from pcrcg_amd.pyramid import build_pyramid  # noqa: E402
from pcrcg_amd.train_forward import forward_train  # noqa: E402

LIMITS = [43, 42, 47, 43]       # tests/golden/calibration.json, S30k
ROOFLINE = 8.0e12               # bytes / s


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


def folding(net, x, upto=None):
    layers = [m for m in net.folding1 if isinstance(m, nn.Linear)][:upto]
    for layer in layers:
        x = torch.relu_(ops.gemm(x, layer.weight.data.t(), bias=layer.bias.data))
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--train-calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_heads.py needs a HIP device")
    dev = torch.device("cuda:0")
    nets = {}
    for name, flags in (("plain", {}), ("heads", dict(node_overlap=True, quaternion=True))):
        torch.manual_seed(0)
        np.random.seed(0)
        nets[name] = KPFCNN(indoor_config(**flags)).to(dev)
        nets[name].use_runner = False                      # both on the op-by-op path: the difference is the heads
    cfg = indoor_config()
    src, tgt = synthetic.pair("S30k", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(dev)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=dev)
    batch = build_pyramid(pts, lens, cfg, LIMITS)
    batch["features"] = torch.ones((pts.shape[0], 1), device=dev)
    n = int(pts.shape[0])
    net = nets["heads"]

    with torch.no_grad():
        feats_f = net.eval().forward_ops(batch)["feats_f"]
        h4 = folding(net, feats_f, upto=4)
        h = folding(net, feats_f)
        last = [m for m in net.folding1 if isinstance(m, nn.Linear)][-1]
        lin1, lin2 = net.linear1, net.linear2
        q_rows = ops.pose_head(h, lin1.weight.data, lin1.bias.data, lin2.weight.data, lin2.bias.data, want_rows=True)[2]
        g = torch.randn(7, device=dev)
        dh = torch.empty_like(h)
        fns = {"forward_ops_plain": lambda: nets["plain"].eval().forward_ops(batch),
               "forward_ops_heads": lambda: net.forward_ops(batch),
               "folding_chain": lambda: folding(net, feats_f),
               "last_folding_layer": lambda: torch.relu_(ops.gemm(h4, last.weight.data.t(), bias=last.bias.data)),
               "tail": lambda: ops.pose_head(h, lin1.weight.data, lin1.bias.data, lin2.weight.data, lin2.bias.data),
               "tail_with_rows": lambda: ops.pose_head(h, lin1.weight.data, lin1.bias.data, lin2.weight.data, lin2.bias.data,
                                                       want_rows=True),
               "tail_backward": lambda: ops.pose_head_backward(h, lin1.weight.data, lin2.weight.data, q_rows, g, dh=dh)}
        t = timed(fns, args.calls, args.repeats, args.warmup)

    def train_step(model):
        model.train()
        out = forward_train(model, batch)
        sum(v.sum() for v in out.values()).backward()
        for p in model.parameters():
            p.grad = None

    t.update(timed({"train_plain": lambda: train_step(nets["plain"]), "train_heads": lambda: train_step(net)},
                   args.train_calls, args.repeats, 1))
    h_bytes = n * 1024 * 4
    tail_bytes = {"tail": h_bytes + 7 * 1024 * 4, "tail_with_rows": h_bytes + 7 * 1024 * 4 + n * 16,
                  "tail_backward": 2 * h_bytes + n * 16 + 7 * 1024 * 4}
    roof = {k: dict(bytes=b, tb_per_s=round(b / (t[k][0] * 1e-6) / 1e12, 2), share_of_8tb_per_s=round(b / (t[k][0] * 1e-6) / ROOFLINE, 3))
            for k, b in tail_bytes.items()}
    heads_us = t["forward_ops_heads"][0] - t["forward_ops_plain"][0]
    print(json.dumps(dict(points=n, coarse_rows=int(batch["points"][-1].shape[0]), h_megabytes=round(h_bytes / 1e6, 1),
                          us_per_call_median_min_max=t, tail_roofline=roof, heads_in_forward_us=round(heads_us, 1),
                          # the write of h by the last folding layer and its read by the tail: what a fused kernel could save
                          h_write_and_read_share_of_heads=round((t["last_folding_layer"][0] + t["tail"][0]) / max(heads_us, 1e-9), 3),
                          h_write_and_read_share_of_forward=round((t["last_folding_layer"][0] + t["tail"][0]) / t["forward_ops_heads"][0], 3))),
          flush=True)


if __name__ == "__main__":
    main()
