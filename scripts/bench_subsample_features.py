"""Time grid subsampling with features / classes on the S30k level-0 shape (2 x 30 000 points, dl = 0.025 * 2).

The points-only call (pcrcg_grid_subsample_batch) and pcrcg_grid_subsample_batch_ex with fdim in {3, 32, 128} and with
ldim = 1 are launched through the C ABI on preallocated buffers -- no host read-back inside the timed window -- and timed
with HIP event pairs around `--calls` back-to-back calls, after warm-up; the configurations alternate inside every
repeat, and the median over `--repeats` is reported.  The feature pass is not timed by itself: its time is the median
call time with features minus the points-only one, and the bytes counted for it are what the algorithm has to move,
N * fdim * 4 read plus M * fdim * 4 written.  Needs a GPU; prints one JSON line.

    python scripts/bench_subsample_features.py [--calls 20] [--repeats 15] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pcrcg_amd import _lib, synthetic  # noqa: E402

DL = 0.025 * 2
CONFIGS = [("points_only", 0, 0), ("fdim3", 3, 0), ("fdim32", 32, 0), ("fdim128", 128, 0), ("ldim1", 0, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    src, tgt = synthetic.pair("S30k", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt]).astype(np.float32)).to(dev)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=dev)
    n, nb = pts.shape[0], 2
    g = torch.Generator(device="cpu").manual_seed(0)
    feats = torch.randn(n, 128, generator=g).to(dev)
    classes = torch.randint(0, 20, (n,), generator=g, dtype=torch.int32).to(dev)
    out_p = torch.empty(n, 3, device=dev)
    out_f = torch.empty(n, 128, device=dev)
    out_c = torch.empty(n, dtype=torch.int32, device=dev)
    out_len = torch.empty(nb, dtype=torch.int32, device=dev)
    out_m = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = L.pcrcg_grid_subsample_ex_ws_bytes(n, nb, 128, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    # the narrow feature matrices are made once, outside the timed windows
    narrow = {fdim: feats[:, :fdim].contiguous() for _, fdim, _ in CONFIGS if fdim}

    def call(fdim, ldim):
        if fdim == 0 and ldim == 0:
            rc = L.pcrcg_grid_subsample_batch(pts.data_ptr(), n, lens.data_ptr(), nb, DL, 0, out_p.data_ptr(), out_len.data_ptr(),
                                              out_m.data_ptr(), ws.data_ptr(), nbytes, stream)
        else:
            rc = L.pcrcg_grid_subsample_batch_ex(pts.data_ptr(), n, lens.data_ptr(), nb, DL, 0,
                                                 narrow[fdim].data_ptr() if fdim else None, fdim, fdim,
                                                 classes.data_ptr() if ldim else None, ldim, out_p.data_ptr(),
                                                 out_len.data_ptr(), out_m.data_ptr(), out_f.data_ptr() if fdim else None,
                                                 out_c.data_ptr() if ldim else None, ws.data_ptr(), nbytes, stream)
        if rc != 0:
            _lib.check(rc, "grid subsample")

    def timed(fdim, ldim):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.calls):
            call(fdim, ldim)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.calls          # microseconds per call

    for _ in range(a.warmup):
        for _, fdim, ldim in CONFIGS:
            call(fdim, ldim)
    torch.cuda.synchronize()
    m = int(out_m.item())
    times = {name: [] for name, _, _ in CONFIGS}
    for _ in range(a.repeats):
        for name, fdim, ldim in CONFIGS:
            times[name].append(timed(fdim, ldim))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: [min(v), max(v)] for k, v in times.items()}
    feat_us = med["fdim128"] - med["points_only"]
    moved = (n + m) * 128 * 4
    print(json.dumps({"shape": "S30k level 0", "points": n, "rows": m, "dl": DL, "calls_per_window": a.calls, "repeats": a.repeats,
                      "median_us_per_call": {k: round(v, 2) for k, v in med.items()},
                      "min_max_us_per_call": {k: [round(x, 2) for x in v] for k, v in spread.items()},
                      "fdim128_feature_pass": {"us": round(feat_us, 2), "bytes": moved,
                                               "GB_per_s": round(moved / (feat_us * 1e-6) / 1e9, 1) if feat_us > 0 else None}}))


if __name__ == "__main__":
    main()
