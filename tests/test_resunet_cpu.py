"""CPU: the 2-D backbone's module tree, initialisation, checkpoint loading and argument checks, and the float64 oracle
(tests/resunet_ref.py) against the reference's fixtures (scripts/make_golden_resunet.py)."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

from pcrcg_amd import resunet
from tests import resunet_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _image(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, h, w, generator=g, dtype=torch.float64) * 2.0 - 1.0


def test_state_dict_names_shapes_and_seed0_digests():
    ref = json.load(open(os.path.join(GOLDEN, "res50unet_keys.json")))
    torch.manual_seed(0)
    m = resunet.Res50UNet(128)
    sd = m.state_dict()
    assert len(sd) == resunet.N_TENSORS == len(ref["tensors"])
    for (k, v), r in zip(sd.items(), ref["tensors"]):
        assert k == r["name"]
        assert list(v.shape) == r["shape"], k
        assert hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() == r["sha256"], k


def test_build_backbone_and_pretrained_refusals():
    m = resunet.build_backbone("Res50UNet", 16)
    assert isinstance(m, resunet.Res50UNet) and m.decoder.conv0.out_channels == 16
    with pytest.raises(NotImplementedError, match="Res50UNet"):
        resunet.build_backbone("Res18UNet", 128)
    for p in ("imagenet", True, "mocov2"):
        with pytest.raises(ValueError, match="checkpoint"):
            resunet.Res50UNet(128, pretrained=p)
        with pytest.raises(ValueError, match="checkpoint"):
            resunet.build_backbone("Res50UNet", 128, pretrained=p)


def test_load_checkpoint_keeps_matching_names_and_shapes(tmp_path):
    torch.manual_seed(3)
    src = resunet.Res50UNet(128)
    torch.manual_seed(4)
    dst = resunet.Res50UNet(128)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    ck = {"backbone." + k: v for k, v in src.state_dict().items() if k.startswith("encoder.layer1.")}
    ck["backbone.not.a.key"] = torch.zeros(3)
    ck["backbone.decoder.conv0.weight"] = torch.zeros(7, 128, 1, 1)          # wrong shape: skipped
    path = tmp_path / "ck.pth"
    torch.save({"model": ck, "epoch": 1}, path)
    loaded = resunet.load_checkpoint(dst, str(path))
    want = sorted(k for k in src.state_dict() if k.startswith("encoder.layer1."))
    assert loaded == want
    after = dst.state_dict()
    for k, v in after.items():
        if k in want:
            assert torch.equal(v, src.state_dict()[k]), k
        else:
            assert torch.equal(v, before[k]), k


def test_oracle_matches_reference_small():
    g = torch.load(os.path.join(GOLDEN, "res50unet_small.pt"))
    torch.manual_seed(0)
    m = resunet.Res50UNet(128)
    sd = m.state_dict()
    x = _image(g["image_seed"], g["h"], g["w"])
    y, run = resunet_ref.resunet_forward(sd, x, training=True, joint=True)
    assert list(y.shape) == g["shape"] == [1, 128, *resunet.output_size(g["h"], g["w"])]
    ref = g["train_out"]
    assert (y.flatten()[::g["stride"]] - ref).abs().max() <= 1e-9 * max(1.0, ref.abs().max())
    for k, v in g["running"].items():
        name, which = k.rsplit(".", 1)
        got = run[name][0 if which == "running_mean" else 1].float()
        assert torch.allclose(got, v, rtol=1e-6, atol=1e-7), k
    resunet_ref.recipe(m, seed=g["recipe_seed"])
    ye, _ = resunet_ref.resunet_forward(m.state_dict(), x, training=False)
    ref = g["eval_out"]
    assert (ye.flatten()[::g["stride"]] - ref).abs().max() <= 1e-9 * max(1.0, ref.abs().max())


def test_oracle_matches_reference_240x320():
    g = torch.load(os.path.join(GOLDEN, "res50unet_240x320.pt"))
    torch.manual_seed(0)
    sd = resunet.Res50UNet(128).state_dict()
    y, _ = resunet_ref.resunet_forward(sd, _image(g["image_seed"], g["h"], g["w"]), training=True)
    assert list(y.shape) == g["shape"] == [1, 128, 120, 160]
    ref = g["out"]
    assert (y.flatten()[::g["stride"]] - ref).abs().max() <= 1e-9 * max(1.0, ref.abs().max())
    assert (y.mean(dim=(0, 2, 3)) - g["channel_means"]).abs().max() <= 1e-9


def test_oracle_matches_reference_odd_and_one_pixel_high():
    """17 x 33 (odd at every halving; layer4 holds 2 values) in training mode and 1 x 9 (every map 1 pixel high, the resize
    at H == 1 and OH == 1) in eval mode: the shapes tests/test_resunet_edges_gpu.py runs the HIP path at."""
    g = torch.load(os.path.join(GOLDEN, "res50unet_odd.pt"))
    torch.manual_seed(0)
    m = resunet.Res50UNet(128)
    t = g["train"]
    y, run = resunet_ref.resunet_forward(m.state_dict(), _image(t["image_seed"], t["h"], t["w"]), training=True)
    assert list(y.shape) == t["shape"] == [1, 128, *resunet.output_size(t["h"], t["w"])] == [1, 128, 10, 18]
    # layer4's BatchNorms see 2 values each, and the network is ill-conditioned there: moving the image by 1e-15 relative
    # moves this output by 5.5e-8, so float64 rounding alone separates two correct runs by that much.  A wrong shape rule
    # (a floor for a ceil, the resize's corners) is an O(1) change.
    ref = t["out"]
    assert (y.flatten()[::t["stride"]] - ref).abs().max() <= 1e-6 * max(1.0, ref.abs().max())
    assert len(t["running"]) == 2 * len(run)
    for k, v in t["running"].items():
        name, which = k.rsplit(".", 1)
        got = run[name][0 if which == "running_mean" else 1].float()
        assert torch.allclose(got, v, rtol=1e-6, atol=1e-7), k
    e = g["eval"]
    resunet_ref.recipe(m, seed=e["recipe_seed"])
    ye, _ = resunet_ref.resunet_forward(m.state_dict(), _image(e["image_seed"], e["h"], e["w"]), training=False)
    assert ye.shape == e["out"].shape == (1, 128, *resunet.output_size(e["h"], e["w"])) == (1, 128, 2, 6)
    assert (ye - e["out"]).abs().max() <= 1e-9 * max(1.0, e["out"].abs().max())


def test_arena_bytes_follow_out_ch():
    from pcrcg_amd import _lib
    L = _lib.lib()
    m = resunet.Res50UNet(128)
    body = sum(v.numel() for k, v in m.state_dict().items() if v.dim() == 4 and not k.startswith("decoder.conv0"))
    for oc in (1, 3, 64, 65, 200, 4096):
        assert L.pcrcg_res50unet_arena_bytes(oc) == 4 * (body + 128 * oc + oc + 64 * 13), oc
    assert L.pcrcg_res50unet_arena_bytes(4097) == 0


def test_abi_rejects_bad_arguments_without_a_device():
    from pcrcg_amd import _lib
    L = _lib.lib()
    assert L.pcrcg_res50unet_arena_bytes(0) == 0
    m = resunet.Res50UNet(128)
    n_conv = sum(v.numel() for k, v in m.state_dict().items() if v.dim() == 4) + 128
    # the derived copy: every convolution weight once (the stem padded from 147 to 160 taps) and the last bias
    assert L.pcrcg_res50unet_arena_bytes(128) == 4 * (n_conv + 64 * 13)
    assert L.pcrcg_res50unet_ws_bytes(0, 240, 320) == 0
    assert L.pcrcg_res50unet_ws_bytes(4, 0, 320) == 0
    assert L.pcrcg_res50unet_ws_bytes(4, 240, 320) > 0
    table = (ctypes.c_void_p * resunet.N_TENSORS)(*([16] * resunet.N_TENSORS))
    p = ctypes.c_void_p(16)
    ws = L.pcrcg_res50unet_ws_bytes(1, 72, 88)
    EBADARG = -1
    assert L.pcrcg_res50unet_pack(None, resunet.N_TENSORS, 128, p, None) == EBADARG
    assert L.pcrcg_res50unet_pack(table, 391, 128, p, None) == EBADARG
    assert L.pcrcg_res50unet_pack(table, resunet.N_TENSORS, 0, p, None) == EBADARG
    args = dict(arena=p, state=table, nt=resunet.N_TENSORS, oc=128, im=p, n=1, h=72, w=88, joint=0, train=1, out=p, ws=p,
                wsb=ws)

    def fwd(**kw):
        a = dict(args, **kw)
        return L.pcrcg_res50unet_forward(a["arena"], a["state"], a["nt"], a["oc"], a["im"], a["n"], a["h"], a["w"],
                                         a["joint"], a["train"], a["out"], a["ws"], a["wsb"], None)
    assert fwd(arena=None) == EBADARG
    assert fwd(state=None) == EBADARG
    assert fwd(nt=10) == EBADARG
    assert fwd(n=0) == EBADARG
    assert fwd(h=0) == EBADARG
    assert fwd(joint=2) == EBADARG
    assert fwd(train=5) == EBADARG
    assert fwd(im=None) == EBADARG
    # one image of 8 x 8: layer4 is 1 x 1, a batch-of-one statistic of a single value (torch refuses it too)
    assert fwd(h=8, w=8) == EBADARG
    # the statistics limit, just past it in each mode: layer4 is ceil(h / 32) x ceil(w / 32)
    assert fwd(h=32, w=32, joint=1) == EBADARG             # joint, one image of one value
    assert fwd(n=2, h=32, w=32, joint=0) == EBADARG        # per image: two images of one value each
    assert fwd(n=3, h=1, w=32, joint=0) == EBADARG
    # the size limits: h, w <= 8192, n <= 65535, n ceil(h / 2) ceil(w / 2) 160 < 2^31
    assert L.pcrcg_res50unet_ws_bytes(1, 1, 8192) > 0 and L.pcrcg_res50unet_ws_bytes(1, 8192, 1) > 0
    assert L.pcrcg_res50unet_ws_bytes(1, 1, 8193) == 0 and L.pcrcg_res50unet_ws_bytes(1, 8193, 1) == 0
    assert L.pcrcg_res50unet_ws_bytes(1, 8192, 6552) > 0 and L.pcrcg_res50unet_ws_bytes(1, 8192, 6553) == 0
    assert L.pcrcg_res50unet_ws_bytes(65535, 1, 1) > 0 and L.pcrcg_res50unet_ws_bytes(65536, 1, 1) == 0
    assert fwd(h=1, w=8193, train=0) == EBADARG
    assert fwd(n=65536, h=1, w=1, train=0) == EBADARG
    assert fwd(wsb=ws - 1) == -2          # PCRCG_EWORKSPACE, still before any launch
    assert "workspace" in L.pcrcg_last_error().decode()
