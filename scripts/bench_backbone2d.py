"""PCR-CG's 2-D backbone Res50UNet(128): the HIP path (pcrcg_amd.resunet, csrc/conv2d.hip) against the reference's
formulation run by torch fp32 on the same GPU (what users run today: one batch-of-one call per image, training-mode
BatchNorm, ref:models/architectures.py:278-281).

Prints one JSON line: ms per image and per shipped pair (4 images of 240 x 320 in one forward_images call), device-event
timed after warm-up; the fp32-equivalent TF/s over the convolutions' FLOPs (counted here from the shapes); the torch fp32
yardstick.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_backbone2d.py`.

usage: python scripts/bench_backbone2d.py [--steps 10] [--warmup 3] [--no-torch]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcrcg_amd import resunet  # noqa: E402


def conv_flops(model, h, w):
    """2 * MACs of every convolution of one h x w image (shapes only)."""
    total = 0

    def hook(mod, inp, out):
        nonlocal total
        total += 2 * out.numel() // out.shape[0] * mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
    import copy
    model = copy.deepcopy(model).to("meta").eval()
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        _torch_forward(model, torch.zeros(1, 3, h, w, device="meta"))
    for hd in hs:
        hd.remove()
    return total


def _torch_forward(m, x):
    """The reference's Res50UNet forward as torch modules (training-mode BatchNorm on the batch)."""
    e = m.encoder
    x = e.maxpool(e.relu(e.bn1(e.conv1(x))))
    feats = []
    for L in (e.layer1, e.layer2, e.layer3, e.layer4):
        for b in L:
            o = b.relu(b.bn1(b.conv1(x)))
            o = b.relu(b.bn2(b.conv2(o)))
            o = b.bn3(b.conv3(o))
            x = b.relu(o + (b.downsample(x) if b.downsample is not None else x))
        feats.append(x)
    x = feats[3]
    for u, up in enumerate((m.decoder.up1, m.decoder.up2, m.decoder.up3, m.decoder.up4)):
        size = feats[2 - u].shape[2:] if u < 3 else (feats[0].shape[2] * 2, feats[0].shape[3] * 2)
        x = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)
        x = up.relu(up.bn1_2(up.conv1_2(up.relu(up.bn1(up.conv1(x))))) + up.bn2(up.conv2(x)))
        if u < 3:
            x = x + feats[2 - u]
    return m.decoder.conv0(x)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = resunet.Res50UNet(128)
    flops = conv_flops(m, 240, 320)
    m = m.to(dev).train()
    x4 = torch.rand(4, 3, 240, 320, device=dev) * 2 - 1
    res = {"gflop_per_image": round(flops / 1e9, 2)}
    with torch.no_grad():
        ms_pair = timed(lambda: m.forward_images(x4), args.steps, args.warmup)
        ms_one = timed(lambda: m.forward_images(x4[:1]), args.steps, args.warmup)
    res.update(hip_ms_per_pair=round(ms_pair, 3), hip_ms_per_image_in_pair=round(ms_pair / 4, 3),
               hip_ms_single_image=round(ms_one, 3), hip_tflops_fp32_equiv=round(4 * flops / ms_pair / 1e9, 1),
               hip_share_of_fp16_two_term_peak=round(4 * flops / ms_pair / 1e9 / (2500.0 / 3), 3))
    if not args.no_torch:
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False
        with torch.no_grad():
            ms_t = timed(lambda: [_torch_forward(m, x4[i:i + 1]) for i in range(4)], args.steps, args.warmup)
        res.update(torch_fp32_ms_per_pair=round(ms_t, 3), torch_fp32_tflops=round(4 * flops / ms_t / 1e9, 1),
                   speedup_vs_torch=round(ms_t / ms_pair, 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
