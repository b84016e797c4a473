"""tests/golden/res50unet_*: PCR-CG's 2-D backbone Res50UNet(128) from the UNMODIFIED reference (build container only).

  res50unet_keys.json     state_dict names, shapes and the sha256 of every tensor of the model built under
                          torch.manual_seed(0) (float32 bytes; num_batches_tracked as int64)
  res50unet_small.pt      72 x 88 (odd halvings: 36 x 44, 18 x 22, 9 x 11, 5 x 6, 3 x 3), seed-0 weights, image from
                          torch.manual_seed(1): the reference run in float64 in training mode (batch of one) -- every 5th
                          output element and the running buffers after the call (float32) -- and, after
                          tests/resunet_ref.recipe (negative gammas, non-trivial running statistics), its eval-mode output
                          (every 5th element)
  res50unet_240x320.pt    240 x 320, seed-0 weights, image from torch.manual_seed(2), training mode: every 97th output
                          element and the per-channel means (float64)
  res50unet_odd.pt        the shapes the two above do not reach, seed-0 weights: 17 x 33 (odd at every halving, layer4
                          1 x 2) in training mode, image from torch.manual_seed(3), every 3rd output element and the
                          running buffers after the call (float32); and 1 x 9 (1-pixel-high maps all the way down, the
                          bilinear resize with H == 1 and OH == 1) in eval mode after tests/resunet_ref.recipe(seed=1),
                          image from torch.manual_seed(4), the whole output

python scripts/make_golden_resunet.py [odd]: all fixtures, or only res50unet_odd.pt
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

OUT = os.path.join(ref_import.REPO, "tests", "golden")


def image(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, h, w, generator=g, dtype=torch.float64) * 2.0 - 1.0


def main():
    ref_import.setup()
    sys.path.insert(0, os.path.join(ref_import.REPO, "tests"))
    from models.resunet import Res50UNet
    import resunet_ref
    torch.set_num_threads(os.cpu_count())
    torch.manual_seed(0)
    m = Res50UNet(128, pretrained=False)
    keys = []
    for k, v in m.state_dict().items():
        keys.append({"name": k, "shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", ""),
                     "sha256": hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest()})
    with open(os.path.join(OUT, "res50unet_keys.json"), "w") as f:
        json.dump({"seed": 0, "output_channel": 128, "tensors": keys}, f, indent=0)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}

    # small: training, then the recipe in eval mode
    md = Res50UNet(128, pretrained=False).double()
    md.load_state_dict(sd0)
    md.train()
    x = image(1, 72, 88)
    with torch.no_grad():
        y = md(x)
    running = {k: v.float() for k, v in md.state_dict().items() if k.endswith("running_mean") or k.endswith("running_var")}
    resunet_ref.recipe(md, seed=1)
    md.eval()
    with torch.no_grad():
        ye = md(x)
    torch.save({"h": 72, "w": 88, "image_seed": 1, "recipe_seed": 1, "stride": 5, "train_out": y.flatten()[::5].clone(),
                "shape": list(y.shape), "running": running, "eval_out": ye.flatten()[::5].clone()},
               os.path.join(OUT, "res50unet_small.pt"))

    md = Res50UNet(128, pretrained=False).double()
    md.load_state_dict(sd0)
    md.train()
    x = image(2, 240, 320)
    with torch.no_grad():
        y = md(x)
    torch.save({"h": 240, "w": 320, "image_seed": 2, "stride": 97, "out": y.flatten()[::97].clone(),
                "shape": list(y.shape), "channel_means": y.mean(dim=(0, 2, 3)).clone()},
               os.path.join(OUT, "res50unet_240x320.pt"))
    for f in ("res50unet_keys.json", "res50unet_small.pt", "res50unet_240x320.pt"):
        print(f, os.path.getsize(os.path.join(OUT, f)))
    odd()


def odd():
    ref_import.setup()
    sys.path.insert(0, os.path.join(ref_import.REPO, "tests"))
    from models.resunet import Res50UNet
    import resunet_ref
    torch.set_num_threads(os.cpu_count())
    torch.manual_seed(0)
    m = Res50UNet(128, pretrained=False)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    md = Res50UNet(128, pretrained=False).double()
    md.load_state_dict(sd0)
    md.train()
    x = image(3, 17, 33)
    with torch.no_grad():
        y = md(x)
    running = {k: v.float() for k, v in md.state_dict().items() if k.endswith("running_mean") or k.endswith("running_var")}
    md = Res50UNet(128, pretrained=False).double()
    md.load_state_dict(sd0)
    resunet_ref.recipe(md, seed=1)
    md.eval()
    xe = image(4, 1, 9)
    with torch.no_grad():
        ye = md(xe)
    torch.save({"train": {"h": 17, "w": 33, "image_seed": 3, "stride": 3, "out": y.flatten()[::3].clone(),
                          "shape": list(y.shape), "running": running},
                "eval": {"h": 1, "w": 9, "image_seed": 4, "recipe_seed": 1, "out": ye.clone()}},
               os.path.join(OUT, "res50unet_odd.pt"))
    print("res50unet_odd.pt", os.path.getsize(os.path.join(OUT, "res50unet_odd.pt")))


if __name__ == "__main__":
    odd() if sys.argv[1:] == ["odd"] else main()
