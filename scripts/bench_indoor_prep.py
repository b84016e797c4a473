"""Preparing 3DMatch pairs on one GPU (pcrcg_amd/indoor.py): prints ONE JSON line.

Workload: B = 8 S30k-shaped LoMatch pairs (synthetic.lomatch_pair("S30k", seed, 0.2): about 30 000 points a side) with two
480 x 640 frames per side, i.e. 32 colour and 32 depth frames.  Host clock around a device synchronise, one warm-up, the
median of --reps calls.

  frames_ms        : prepare_frames, the 64 host frames in ONE upload and ONE pcrcg_prepare_frames call
  frames_device_ms : the same call with the frames already on the device (no upload)
  frames_torch_ms  : the same conversion as torch indexing on the device, from the uploaded frames (index tables precomputed;
                     its values are compared with the kernel's and the largest difference is printed)
  frames_pil_ms    : PIL's resize + the ToTensor arithmetic in numpy on this host's CPU (None where PIL is absent)
  corr_batch_ms    : get_correspondences_batch on the 8 pairs
  corr_loop_ms     : eight get_correspondences calls (the code kitti.prepare_pairs loops over)
The two correspondence timings are interleaved call by call in one process (--reps, default 20).  The kernel's frames are
compared with the numpy restatement and the two correspondence results with each other (bit for bit) before anything is
timed.  Recorded figures: DESIGN.md section 15."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcrcg_amd import indoor, synthetic  # noqa: E402
from pcrcg_amd.correspondences import get_correspondences, get_correspondences_batch  # noqa: E402
from tests import indoor_ref as IR  # noqa: E402


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.pairs
    rng = np.random.RandomState(0)
    colours = [rng.randint(0, 256, (480, 640, 3)).astype(np.uint8) for _ in range(4 * B)]
    depths = [rng.randint(0, 65536, (480, 640)).astype(np.uint16) for _ in range(4 * B)]
    out = {"metric": "indoor_prep", "device": torch.cuda.get_device_name(0), "reps": a.reps, "pairs": B,
           "frames": [len(colours), len(depths)]}

    # ---- frames ----
    c, d = indoor.prepare_frames(colours, depths)                                       # warm-up, and the comparison
    same = c[3].cpu().numpy().tobytes() == IR.color_to_tensor(colours[3], (240, 320)).tobytes() and \
        d[5].cpu().numpy().tobytes() == IR.depth_to_tensor(depths[5], (120, 160)).tobytes()
    cu = torch.from_numpy(np.stack(colours)).to(dev)
    du = torch.from_numpy(np.stack(depths).view(np.int16)).to(dev)
    iy, ix = (torch.from_numpy(IR.nearest_index(n, m)).to(dev) for n, m in ((480, 240), (640, 320)))
    jy, jx = (torch.from_numpy(IR.nearest_index(n, m)).to(dev) for n, m in ((480, 120), (640, 160)))

    def by_torch():
        tc = cu[:, iy][:, :, ix].permute(0, 3, 1, 2).float() / 255.0
        td = du[:, jy][:, :, jx].float() / 1000.0
        return tc.contiguous(), td

    tc, td = by_torch()
    out["frames_equal_restatement"] = bool(same)
    # (torch divides a device tensor by a Python scalar as a multiplication by its reciprocal: the last bit may differ)
    out["frames_torch_equal"] = bool(torch.equal(tc, c) and torch.equal(td, d))
    out["frames_torch_max_abs_diff"] = [float((tc - c).abs().max()), float((td - d).abs().max())]
    reps_f = min(a.reps, 9)
    out["frames_ms"] = round(1e3 * float(np.median([clock(lambda: indoor.prepare_frames(colours, depths)) for _ in range(reps_f)])), 3)
    cd, dd = list(cu), list(du)
    indoor.prepare_frames(cd, dd)
    out["frames_device_ms"] = round(1e3 * float(np.median([clock(lambda: indoor.prepare_frames(cd, dd)) for _ in range(reps_f)])), 3)
    out["frames_torch_ms"] = round(1e3 * float(np.median([clock(by_torch) for _ in range(reps_f)])), 3)
    try:
        from PIL import Image

        def by_pil():
            for f in colours:
                np.asarray(Image.fromarray(f).resize((320, 240), Image.NEAREST)).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
            for f in depths:
                np.asarray(Image.fromarray(f).resize((160, 120), Image.NEAREST)).view(np.int16).astype(np.float32) / np.float32(1000)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            by_pil()
            ts.append(time.perf_counter() - t0)
        out["frames_pil_ms"] = round(1e3 * float(np.median(ts)), 3)
    except ImportError:
        out["frames_pil_ms"] = None

    # ---- correspondences ----
    src, tgt, Ts = [], [], []
    for s in range(B):
        p, q, rot, trans = synthetic.lomatch_pair("S30k", s, 0.2)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = rot, trans.flatten()
        src.append(torch.from_numpy(p).to(dev))
        tgt.append(torch.from_numpy(q).to(dev))
        Ts.append(T)
    loop = lambda: [get_correspondences(s, t, T, 0.0375) for s, t, T in zip(src, tgt, Ts)]
    batch = lambda: get_correspondences_batch(src, tgt, Ts, 0.0375)
    one, many = loop(), batch()
    out["corr_bit_identical"] = all(torch.equal(x, y) for x, y in zip(one, many))
    out["n_points"] = [int(sum(x.shape[0] for x in src)), int(sum(x.shape[0] for x in tgt))]
    out["n_correspondences"] = int(sum(x.shape[0] for x in many))
    tb, tl = [], []
    for _ in range(a.reps):                                                             # interleaved, call by call
        tb.append(clock(batch))
        tl.append(clock(loop))
    out["corr_batch_ms"] = round(1e3 * float(np.median(tb)), 3)
    out["corr_loop_ms"] = round(1e3 * float(np.median(tl)), 3)
    out["corr_batch_ms_min_max"] = [round(1e3 * min(tb), 3), round(1e3 * max(tb), 3)]
    out["corr_loop_ms_min_max"] = [round(1e3 * min(tl), 3), round(1e3 * max(tl), 3)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
