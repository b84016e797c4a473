"""GPU: PCR-CG's 2-D backbone Res50UNet on csrc/conv2d.hip against the float64 oracle (tests/resunet_ref.py, itself tied to
the unmodified reference by tests/test_resunet_cpu.py).

The bar is the project's C1 form: the HIP output may be no further from float64 than 3x what the same network run in
plain fp32 on the CPU is, percentile by percentile (p50 / p90 / max of the absolute error)."""
import os

import pytest
import torch

from pcrcg_amd import resunet
from tests import resunet_ref

pytestmark = pytest.mark.gpu


def _image(seed, n, h, w, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, h, w, generator=g, dtype=torch.float64) * 2.0 - 1.0) * scale


def _pct(e):
    e = e.flatten().double()
    return [torch.quantile(e[::max(1, e.numel() // 200000)], q).item() for q in (0.5, 0.9)] + [e.max().item()]


def _meets_bar(got, sd, x, training, joint=True):
    ref, _ = resunet_ref.resunet_forward(sd, x, training=training, joint=joint)
    f32, _ = resunet_ref.resunet_forward(sd, x.float(), training=training, joint=joint, dtype=torch.float32)
    e_gpu = _pct((got.double().cpu() - ref).abs())
    e_f32 = _pct((f32.double() - ref).abs())
    for a, b, q in zip(e_gpu, e_f32, ("p50", "p90", "max")):
        assert a <= 3.0 * b, f"{q}: HIP {a:.3g} vs fp32 CPU {b:.3g} (max|y| {ref.abs().max().item():.3g})"
    return ref


def _model(cuda, seed=0, recipe=None):
    torch.manual_seed(seed)
    m = resunet.Res50UNet(128)
    if recipe is not None:
        resunet_ref.recipe(m, seed=recipe)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to(cuda), sd


def test_accuracy_240x320_training(cuda):
    m, sd = _model(cuda)
    x = _image(2, 1, 240, 320)
    with torch.no_grad():
        y = m(x.float().to(cuda))
    assert y.shape == (1, 128, 120, 160) and y.grad_fn is None
    _meets_bar(y, sd, x, training=True)


@pytest.mark.parametrize("training", [True, False])
def test_affine_recipe_train_and_eval(cuda, training):
    m, sd = _model(cuda, recipe=1)
    m.train(training)
    x = _image(1, 1, 72, 88)
    y = m(x.float().to(cuda))
    assert y.shape == (1, 128, 36, 44)
    _meets_bar(y, sd, x, training=training)


def test_per_image_statistics_and_running_buffers(cuda):
    m, sd = _model(cuda, recipe=1)
    x = _image(5, 4, 72, 88)
    nbt0 = m.encoder.bn1.num_batches_tracked.item()
    y4 = m.forward_images(x.float().to(cuda))
    torch.cuda.synchronize()
    after = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert m.encoder.bn1.num_batches_tracked.item() == nbt0 + 4
    assert m.decoder.up4.bn2.num_batches_tracked.item() == nbt0 + 4
    # the oracle's four sequential batch-of-one updates; the buffers are statistics of activations that carry the forward's
    # fp32-class error, so the bar is 1e-6 relative or 3x the plain-fp32 CPU run's error, whichever is larger
    _, run = resunet_ref.resunet_forward(sd, x, training=True, joint=False)
    _, run32 = resunet_ref.resunet_forward(sd, x.float(), training=True, joint=False, dtype=torch.float32)
    for name, (rm, rv, k) in run.items():
        assert k == 4
        for i, (got, want) in enumerate(((after[name + ".running_mean"], rm), (after[name + ".running_var"], rv))):
            e32 = (run32[name][i].double() - want).abs().max().item()
            bar = max(1e-6 * max(1.0, want.abs().max().item()), 3.0 * e32)
            assert (got.double() - want).abs().max().item() <= bar, name
    # four single-image calls from the same starting state give the same maps
    m1, _ = _model(cuda, recipe=1)
    singles = torch.cat([m1.forward_images(x[i:i + 1].float().to(cuda)) for i in range(4)])
    assert (singles - y4).abs().max().item() <= 1e-6 * y4.abs().max().item()
    for i in range(4):
        _meets_bar(y4[i:i + 1], sd, x[i:i + 1], training=True)


def test_joint_statistics_batch_of_two(cuda):
    m, sd = _model(cuda, recipe=1)
    x = _image(6, 2, 72, 88)
    y = m(x.float().to(cuda))
    torch.cuda.synchronize()
    assert m.encoder.bn1.num_batches_tracked.item() == 1
    _meets_bar(y, sd, x, training=True, joint=True)


@pytest.mark.parametrize("scale", [1e5, 1e-9])
def test_range_ends(cuda, scale):
    m, sd = _model(cuda)
    x = _image(7, 1, 72, 88, scale)
    y = m(x.float().to(cuda))
    _meets_bar(y, sd, x, training=True)


def test_kpfcnn_runs_the_pair_images_through_one_backbone_call(cuda, golden_dir):
    """KPFCNN(image_feature=True, img_num=2).forward(batch, backbone2d=Res50UNet): one forward_images call per pair, in the
    reference's order, and the same outputs as the forward fed the oracle's maps."""
    from tests.test_image_gpu import _mini_image_case
    gold, cfg, net, batch = _mini_image_case(cuda, golden_dir, img_num=2)
    bb, sd = _model(cuda, recipe=2)
    bb.eval()                                   # 12 x 16 maps: 24 x 32 images, too small for batch-of-one statistics
    order = [("src", 1), ("src", 2), ("tgt", 1), ("tgt", 2)]
    colors = _image(8, 4, 24, 32)
    b1 = {k: v for k, v in batch.items() if not k.endswith("_feature2d")}
    b2 = dict(b1)
    for (side, i), c in zip(order, colors):
        b1[f"{side}_color{i}"] = c.float().to(cuda)
        fmap, _ = resunet_ref.resunet_forward(sd, c[None], training=False)
        b2[f"{side}{i}_feature2d"] = fmap[0].float().to(cuda)
    calls = []
    real = bb.forward_images
    bb.forward_images = lambda x: (calls.append(x.shape[0]), real(x))[1]
    with torch.no_grad():
        out1 = net(b1, backbone2d=bb)
        out2 = net(b2)
        feats1 = net.image_features(b1, bb)
        feats2 = net.image_features(b2)
    assert calls[0] == 4
    assert (feats1 - feats2).abs().max().item() <= 1e-4 * max(1.0, feats2.abs().max().item())
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        err = ((out1[k] - out2[k]).norm() / out2[k].norm().clamp_min(1e-30)).item()
        assert err < 1e-4, (k, err)
    # a foreign backbone is called once per image, in the reference's order
    seen = []

    def recorder(c):
        seen.append(int(round(float(c.flatten()[0]))))
        return torch.zeros(1, 128, 12, 16, device=cuda)
    b3 = {k: v for k, v in b1.items()}
    for n, (side, i) in enumerate(order):
        b3[f"{side}_color{i}"] = torch.full((3, 24, 32), float(n), device=cuda)
    with torch.no_grad():
        net.image_features(b3, recorder)
    assert seen == [0, 1, 2, 3]
