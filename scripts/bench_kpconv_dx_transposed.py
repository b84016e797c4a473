"""Time the gather-form backward passes over transposed neighbour tables against the scatter forms, on one MI355X
(DESIGN.md section 19).

The S30k synthetic pair, its pyramid, and every rigid KPConv shape indoor_config() has per level (plain and strided):

  transpose   ops.transpose_neighbors per level and table kind: count + the 8-byte read-back + fill, once per pyramid
  kpconv      scatter:    the d_wf product (pcrcg_gemm_f32_grad) + zeroing dx + pcrcg_kpconv_backward_dx
              transposed: pcrcg_kpconv_backward_dx_t (scale, gather on the transposed table, product), weights pre-permuted
  max_pool    zeroing dx + pcrcg_gather_max_backward    against pcrcg_gather_max_backward_t      (strided shortcuts)
  closest     zeroing dx + pcrcg_gather_first_backward  against pcrcg_gather_first_backward_t    (upsamplings)

each under the default arithmetic and under deterministic=1.  The baseline is the scatter path of the same build.  HIP event
pairs around CALLS back-to-back calls, no read-back inside a window (the transposition's own excepted: it is part of what
is measured), the configurations alternating inside each of REPEATS repeats after a warm-up; median and [min, max] over the
repeats, microseconds per call.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcrcg_amd import _lib, indoor_config, ops, synthetic  # noqa: E402
from pcrcg_amd.architectures import KPFCNN  # noqa: E402
from pcrcg_amd.blocks import NearestUpsampleBlock, ResnetBottleneckBlock, SimpleBlock  # noqa: E402
from pcrcg_amd.pyramid import build_pyramid  # noqa: E402


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


def shapes(net):
    """-> rigid KPConv shapes [(level, strided, cin, cout)], max_pool widths [(level, c)], closest_pool widths [(table, c)]
    of the architecture, each once."""
    convs, pools, ups = [], [], []
    width = None
    for block in net.encoder_blocks:
        if isinstance(block, (SimpleBlock, ResnetBottleneckBlock)):
            strided = "strided" in block.block_name
            conv = block.KPConv
            if conv.rigid:
                convs.append((block.layer_ind, strided, conv.in_channels, conv.out_channels))
            if isinstance(block, ResnetBottleneckBlock):
                if strided:
                    pools.append((block.layer_ind, width))
                width = block.unary2.mlp.weight.shape[0]
            else:
                width = conv.out_channels
    width = net.proj_gnn.out_channels + 2
    for block in net.decoder_blocks:                                 # (a skip joins AFTER the upsampling: not its width)
        if isinstance(block, NearestUpsampleBlock):
            ups.append((block.layer_ind - 1, width))
        elif hasattr(block, "mlp"):
            width = block.mlp.weight.shape[0]
    uniq = lambda xs: sorted(set(xs))
    return uniq(convs), uniq(pools), uniq(ups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kpconv_dx_transposed.py needs a HIP device")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    cfg = indoor_config()
    net = KPFCNN(cfg)
    convs, pools, ups = shapes(net)
    src, tgt = synthetic.pair("S30k", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(dev)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=dev)
    batch = build_pyramid(pts, lens, cfg, synthetic.LIMITS["S30k"])
    n = [int(p.shape[0]) for p in batch["points"]]
    st = ops._stream

    # ---- the transposition, per level and table kind
    tables = {}
    for kind, with_columns in (("neighbors", False), ("pools", True), ("upsamples", False)):
        for l, t in enumerate(batch[kind]):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] == 0:
                continue
            ns = n[l + 1] if kind == "upsamples" else n[l]
            src_t = t[:, :1] if kind == "upsamples" else t
            tr = ops.transpose_neighbors(src_t, ns, with_columns=with_columns)
            tables[(kind, l)] = tr
            tm = timed({"transpose": lambda: ops.transpose_neighbors(src_t, ns, with_columns=with_columns)}, 5, args.repeats,
                       args.warmup)
            nbytes = tr.tq.numel() * 8 + (tr.th.numel() * 4 if tr.th is not None else 0)
            print(json.dumps(dict(what="transpose", table=kind, level=l, nq=int(t.shape[0]), ns=ns, h=int(src_t.shape[1]),
                                  edges=tr.n_edges, d_max=tr.d_max, table_bytes=nbytes, source_bytes=int(src_t.shape[0] * src_t.shape[1] * 8),
                                  us_median_min_max=tm["transpose"])), flush=True)

    for mode in ("default", "deterministic"):
        if mode == "deterministic":
            _lib.check(L.pcrcg_debug_set(b"deterministic=1"), "pcrcg_debug_set")
        try:
            # ---- KPConv d x
            for level, strided, cin, cout in convs:
                s_pts = batch["points"][level]
                q_pts = batch["points"][level + 1] if strided else s_pts
                idx = batch["pools" if strided else "neighbors"][level]
                tr = tables[("pools" if strided else "neighbors", level)]
                nq, h = idx.shape
                ns = s_pts.shape[0]
                r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** level
                extent = r * cfg.KP_extent / cfg.conv_radius
                g = torch.Generator().manual_seed(level * 100 + cin)
                from pcrcg_amd.kernel_points import load_kernels
                kp = torch.tensor(load_kernels(r, 15, dimension=3, fixed="center"), dtype=torch.float32).to(dev)
                w = (torch.randn(15, cin, cout, generator=g) * 0.05).to(dev)
                w2 = w.reshape(15 * cin, cout)
                wt = w.permute(0, 2, 1).reshape(15 * cout, cin).contiguous()
                dy = (torch.randn(nq, cout, generator=g) * 1e-4).to(dev)
                inv_n = (1.0 / torch.randint(1, h + 1, (nq,), generator=g).float()).to(dev)
                dx_s = torch.empty(ns, cin, device=dev)
                dx_t = torch.empty(ns, cin, device=dev)
                nbytes = L.pcrcg_kpconv_backward_dx_t_ws_bytes(nq, ns, cout)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

                def scatter():
                    d_wf = ops.gemm(dy, w2.t(), row_scale=inv_n, grad_operand=1)
                    dx_s.zero_()
                    _lib.check(L.pcrcg_kpconv_backward_dx(q_pts.data_ptr(), nq, s_pts.data_ptr(), ns, idx.data_ptr(), h, idx.stride(0),
                                                          d_wf.data_ptr(), cin, kp.data_ptr(), extent, dx_s.data_ptr(), st()),
                               "pcrcg_kpconv_backward_dx")

                def transposed():
                    _lib.check(L.pcrcg_kpconv_backward_dx_t(q_pts.data_ptr(), nq, s_pts.data_ptr(), ns, tr.tq.data_ptr(),
                                                            tr.tq.shape[1], tr.tq.stride(0), dy.data_ptr(), cout, inv_n.data_ptr(),
                                                            cout, kp.data_ptr(), extent, wt.data_ptr(), cin, dx_t.data_ptr(), cin,
                                                            ws.data_ptr(), nbytes, st()), "pcrcg_kpconv_backward_dx_t")
                tm = timed({"scatter": scatter, "transposed": transposed}, args.calls, args.repeats, args.warmup)
                dev_rel = float((dx_t - dx_s).abs().max() / dx_s.abs().max().clamp(min=1e-30))
                print(json.dumps(dict(what="kpconv_dx", mode=mode, level=level, strided=strided, nq=nq, ns=ns, h=h, cols=tr.d_max,
                                      cin=cin, cout=cout, max_dev_vs_scatter=dev_rel, us_median_min_max=tm,
                                      transposed_over_scatter=round(tm["transposed"][0] / tm["scatter"][0], 3))), flush=True)
            # ---- max_pool (the strided shortcuts)
            for level, c in pools:
                idx = batch["pools"][level]
                tr = tables[("pools", level)]
                nq, h = idx.shape
                ns = n[level]
                g = torch.Generator().manual_seed(level + c)
                x = torch.randn(ns, c, generator=g).to(dev)
                y = ops.gather_max(x, idx)
                dy = (torch.randn(nq, c, generator=g) * 1e-4).to(dev)
                dx_s, dx_t = torch.empty(ns, c, device=dev), torch.empty(ns, c, device=dev)

                def scatter():
                    dx_s.zero_()
                    _lib.check(L.pcrcg_gather_max_backward(x.data_ptr(), ns, c, idx.data_ptr(), nq, h, idx.stride(0), y.data_ptr(),
                                                           dy.data_ptr(), dx_s.data_ptr(), st()), "pcrcg_gather_max_backward")

                def transposed():
                    _lib.check(L.pcrcg_gather_max_backward_t(x.data_ptr(), ns, c, idx.data_ptr(), nq, h, idx.stride(0), y.data_ptr(),
                                                             dy.data_ptr(), tr.tq.data_ptr(), tr.th.data_ptr(), tr.tq.shape[1],
                                                             tr.tq.stride(0), dx_t.data_ptr(), st()), "pcrcg_gather_max_backward_t")
                tm = timed({"scatter": scatter, "transposed": transposed}, args.calls, args.repeats, args.warmup)
                dev_rel = float((dx_t - dx_s).abs().max() / dx_s.abs().max().clamp(min=1e-30))
                print(json.dumps(dict(what="max_pool", mode=mode, level=level, nq=nq, ns=ns, h=h, cols=tr.d_max, c=c,
                                      max_dev_vs_scatter=dev_rel, us_median_min_max=tm,
                                      transposed_over_scatter=round(tm["transposed"][0] / tm["scatter"][0], 3))), flush=True)
            # ---- closest_pool (the upsamplings)
            for table, c in ups:
                idx = batch["upsamples"][table]
                tr = tables[("upsamples", table)]
                nq = idx.shape[0]
                ns = n[table + 1]
                g = torch.Generator().manual_seed(table + c)
                dy = (torch.randn(nq, c, generator=g) * 1e-4).to(dev)
                dx_s, dx_t = torch.empty(ns, c, device=dev), torch.empty(ns, c, device=dev)

                def scatter():
                    dx_s.zero_()
                    _lib.check(L.pcrcg_gather_first_backward(dy.data_ptr(), c, c, idx.data_ptr(), nq, idx.stride(0), ns,
                                                             dx_s.data_ptr(), st()), "pcrcg_gather_first_backward")

                def transposed():
                    _lib.check(L.pcrcg_gather_first_backward_t(dy.data_ptr(), c, c, tr.tq.data_ptr(), tr.tq.shape[1], tr.tq.stride(0),
                                                               nq, ns, dx_t.data_ptr(), c, st()), "pcrcg_gather_first_backward_t")
                tm = timed({"scatter": scatter, "transposed": transposed}, args.calls, args.repeats, args.warmup)
                dev_rel = float((dx_t - dx_s).abs().max() / dx_s.abs().max().clamp(min=1e-30))
                print(json.dumps(dict(what="closest_pool", mode=mode, table=table, nq=nq, ns=ns, cols=tr.d_max, c=c,
                                      max_dev_vs_scatter=dev_rel, us_median_min_max=tm,
                                      transposed_over_scatter=round(tm["transposed"][0] / tm["scatter"][0], 3))), flush=True)
        finally:
            torch.cuda.synchronize()
            if mode == "deterministic":
                _lib.check(L.pcrcg_debug_set(None), "pcrcg_debug_set")
                _lib.check(L.pcrcg_debug_release(), "pcrcg_debug_release")


if __name__ == "__main__":
    main()
