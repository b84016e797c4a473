"""GPU: csrc/conv2d.hip at the edges tests/test_resunet_gpu.py does not reach, against the same float64 oracle
(tests/resunet_ref.py) and the same bar (p50 / p90 / max of |HIP - f64| within 3x the plain-fp32 CPU run's; running buffers
within 1e-6 relative or 3x the fp32 run's error).

  * the per-tile bf16 redo in deep layers: filters far below fp16's normal range (2^-26 .. 2^-23) and far above it (1e5),
    beside tiles of the same product that stay on the fp16 path
  * dead (all-zero) filters and channels whose mean dwarfs their spread
  * out_ch other than 128 (the CHW epilogue at tile widths 64 and 128, partial tiles, its bias)
  * image shapes at the limits of the shape rules: 1-pixel maps, odd sizes, the row-tile edge, the statistics minimum
  * five per-image updates in order; what a call may and may not write
  * deterministic=1: bit-identical outputs and running buffers run after run"""
from unittest import mock

import pytest
import torch

from pcrcg_amd import _lib, resunet
from tests import resunet_ref
from tests.test_resunet_gpu import _image, _meets_bar, _model, _pct

pytestmark = pytest.mark.gpu
EPS = resunet_ref.EPS


def _load(cuda, sd, out_ch=128, training=True):
    m = resunet.Res50UNet(out_ch)
    m.load_state_dict(sd)
    return m.to(cuda).train(training)


def _offset_image(seed, n, h, w):
    return 100.0 + 0.05 * _image(seed, n, h, w)


def _cpu(state):
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in state.items()}


def _running_meets_bar(after, sd, x, joint, pooled=False):
    """The running buffers and counts `after` (a state_dict) holds after one training call on x from state sd, against the
    oracle's: per buffer, 1e-6 relative or 3x the fp32 run's error.  pooled: the errors of all buffers together, p50 / p90 /
    max against 3x the fp32 run's (the output's bar) -- for shapes whose statistics segments hold so few values that the
    network is chaotic (a 1e-7 relative change of the image moves a running mean by up to 0.4 at 1 x 1, by 0.02 at 17 x 33),
    where one buffer's fp32 error is a random draw that may land far below the HIP path's."""
    _, run = resunet_ref.resunet_forward(sd, x, training=True, joint=joint)
    _, run32 = resunet_ref.resunet_forward(sd, x.float(), training=True, joint=joint, dtype=torch.float32)
    updates = 1 if joint else x.shape[0]
    errs, errs32 = [], []
    for name, (rm, rv, k) in run.items():
        assert k == updates
        assert after[name + ".num_batches_tracked"].item() == sd[name + ".num_batches_tracked"].item() + updates, name
        for i, (got, want) in enumerate(((after[name + ".running_mean"], rm), (after[name + ".running_var"], rv))):
            if pooled:
                errs.append((got.double() - want).abs())
                errs32.append((run32[name][i].double() - want).abs())
                continue
            e32 = (run32[name][i].double() - want).abs().max().item()
            bar = max(1e-6 * max(1.0, want.abs().max().item()), 3.0 * e32)
            err = (got.double() - want).abs().max().item()
            assert err <= bar, (name, ("running_mean", "running_var")[i], err, bar)
    if pooled:
        for a, b, q in zip(_pct(torch.cat(errs)), _pct(torch.cat(errs32)), ("p50", "p90", "max")):
            assert a <= 3.0 * b, f"running buffers {q}: HIP {a:.3g} vs fp32 CPU {b:.3g}"


def _bn_inputs(sd, x, training, names, hook=None):
    """Run the oracle (float64, joint statistics) and return {bn name: (channel mean, biased channel variance)} of what it
    feeds each named BatchNorm.  hook(state_dict of the run, bn name, mean, var), when given, is called before that
    BatchNorm runs and may change its parameters for the rest of the run (they are the oracle's own float64 copies)."""
    seen = {}
    real = resunet_ref._State.bn

    def spy(self, name, t):
        if name in names:
            mean, var = t.mean(dim=(0, 2, 3)), t.var(dim=(0, 2, 3), unbiased=False)
            seen[name] = (mean, var)
            if hook is not None:
                hook(self.sd, name, mean, var)
        return real(self, name, t)
    with mock.patch.object(resunet_ref._State, "bn", spy):
        resunet_ref.resunet_forward(sd, x, training=training, joint=True)
    return seen


def _set_filters(sd, conv, chans, seed, lo_exp=None, mag=None):
    """Output channels `chans` of convolution `conv`: signed entries 2^U(lo_exp) (lo_exp = (a, b)) or mag * U(1, 2)."""
    g = torch.Generator().manual_seed(seed)
    w = sd[conv + ".weight"]
    shape = w[chans].shape
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    if lo_exp is not None:
        v = torch.exp2(torch.rand(shape, generator=g, dtype=torch.float64) * (lo_exp[1] - lo_exp[0]) + lo_exp[0])
    else:
        v = mag * (1.0 + torch.rand(shape, generator=g, dtype=torch.float64))
    w[chans] = (sign * v).float()


# convolution -> (its BatchNorm, output channels changed); 72 x 88, one image
REDO_TINY = {
    "encoder.layer1.1.conv3": ("encoder.layer1.1.bn3", [1, 9, 100]),      # 1x1, 396 rows, not split; N-tile 1 stays fp16
    "encoder.layer4.1.conv2": ("encoder.layer4.1.bn2", [3, 17, 40]),      # 3x3, 9 rows, split-K; N-tiles 1..3 stay fp16
    "decoder.up1.conv2": ("decoder.up1.bn2", [5, 70]),                    # 5x5: columns 1029, 1094 of the paired product
}
REDO_LARGE = {
    "encoder.layer1.2.conv1": ("encoder.layer1.2.bn1", [2, 33]),          # 1x1, 396 rows, not split
    "encoder.layer4.0.conv2": ("encoder.layer4.0.bn2", [7, 300]),         # 3x3 stride 2, split-K; N-tiles 1 and 3 stay fp16
}


def test_redo_in_deep_layers_tiny_filters(cuda):
    """Filters of 2^-26 .. 2^-23: fp16 holds them as subnormals or not at all (the two-term split's floor is 2^-36, 2^-13 of
    such a value), so only the tile's bf16 redo (a row of B with nothing at or above 2^-14) keeps them to fp32's error.
    BatchNorm's eps would flatten such channels, so their gamma is raised until the normalised output is O(1) -- and the
    oracle's statistics confirm it, so the case keeps its teeth.  (Without the redo the layer1 channels alone put the output
    3x past the bar; the deep ones move it by less than the bar's width, and are here for the redo's split-K and paired
    forms.)"""
    _, sd = _model(cuda, recipe=1)
    for i, (conv, (_, chans)) in enumerate(REDO_TINY.items()):
        _set_filters(sd, conv, chans, 10 + i, lo_exp=(-26.0, -23.0))
        assert sd[conv + ".weight"][chans].abs().max().item() < 2.0 ** -22
    x = _image(11, 1, 72, 88)
    bns = {bn: chans for bn, chans in REDO_TINY.values()}

    def raise_gamma(osd, name, mean, var):
        c = bns[name]
        osd[name + ".weight"][c] = torch.sqrt(var[c] + EPS) / torch.sqrt(var[c])
        sd[name + ".weight"][c] = osd[name + ".weight"][c].float()
    _bn_inputs(sd, x, True, bns, raise_gamma)
    for name, (mean, var) in _bn_inputs(sd, x, True, bns).items():
        c = bns[name]
        assert var[c].max().item() < 1e-3 * EPS, name                       # eps would flatten the channel ...
        gain = sd[name + ".weight"][c].double().abs() * torch.sqrt(var[c] / (var[c] + EPS))
        assert 0.9 < gain.min().item() and gain.max().item() < 1.1, name    # ... the raised gamma makes it O(1) again
    m = _load(cuda, sd)
    _meets_bar(m(x.float().to(cuda)), sd, x, training=True)


@pytest.mark.parametrize("training", [True, False])
def test_redo_in_deep_layers_large_filters(cuda, training):
    """Filters of +-1e5 .. 2e5: every fp16 product of theirs overflows, so the tile's partial sums go non-finite and the tile
    is redone in bf16.  Training: BatchNorm is scale-invariant per channel.  Eval: those channels' running statistics are
    the oracle's batch statistics of the eval-mode run."""
    _, sd = _model(cuda, recipe=1)
    for i, (conv, (_, chans)) in enumerate(REDO_LARGE.items()):
        _set_filters(sd, conv, chans, 20 + i, mag=1e5)
    x = _image(12, 1, 72, 88)
    bns = {bn: chans for bn, chans in REDO_LARGE.values()}
    if not training:
        def running_from_batch(osd, name, mean, var):
            c = bns[name]
            for key, v in (("running_mean", mean[c]), ("running_var", var[c])):
                osd[f"{name}.{key}"][c] = v
                sd[f"{name}.{key}"][c] = v.float()
        _bn_inputs(sd, x, False, bns, running_from_batch)
        for name, (mean, var) in _bn_inputs(sd, x, False, bns).items():
            c = bns[name]
            assert var[c].min().item() > 1e6, name
            ratio = var[c] / sd[name + ".running_var"][c].double()
            assert 0.99 < ratio.min().item() and ratio.max().item() < 1.01, name
    m = _load(cuda, sd, training=training)
    _meets_bar(m(x.float().to(cuda)), sd, x, training=training)


# convolution -> output channels set to zero: the stem, a 1x1 of layer2, both halves' first columns of up2's paired product
DEAD = {"encoder.conv1": [0, 5], "encoder.layer2.0.conv1": [4, 77], "decoder.up2.conv1": [0, 300],
        "decoder.up2.conv2": [1]}
DEAD_BN = {"encoder.conv1": "encoder.bn1", "encoder.layer2.0.conv1": "encoder.layer2.0.bn1", "decoder.up2.conv1": "decoder.up2.bn1",
           "decoder.up2.conv2": "decoder.up2.bn2"}


@pytest.mark.parametrize("joint", [False, True])
def test_dead_filters(cuda, joint):
    """All-zero filters: the channel's variance is exactly 0, BatchNorm gives beta, and the running buffers decay by the
    momentum once per update."""
    _, sd = _model(cuda, recipe=1)
    for conv, chans in DEAD.items():
        sd[conv + ".weight"][chans] = 0.0
    x = _image(13, 2, 72, 88)
    m = _load(cuda, sd)
    xd = x.float().to(cuda)
    y = m(xd) if joint else m.forward_images(xd)
    if joint:
        _meets_bar(y, sd, x, training=True)
    else:
        for i in range(2):
            _meets_bar(y[i:i + 1], sd, x[i:i + 1], training=True)
    after = _cpu(m.state_dict())
    _running_meets_bar(after, sd, x, joint)
    decay = 0.9 ** (1 if joint else 2)
    for conv, chans in DEAD.items():
        bn = DEAD_BN[conv]
        for key in ("running_mean", "running_var"):
            want = sd[f"{bn}.{key}"][chans].double() * decay
            assert torch.allclose(after[f"{bn}.{key}"][chans].double(), want, rtol=1e-6, atol=0), (bn, key)


def test_mean_far_above_spread_per_image(cuda):
    """Images 100 + 0.05 noise: every channel's mean is thousands of times its spread, the case where a variance taken as
    E[x^2] - E[x]^2 in fp32 loses every digit.  Output and running buffers after two per-image updates."""
    _, sd = _model(cuda, recipe=1)
    x = _offset_image(14, 2, 72, 88)
    m = _load(cuda, sd)
    y = m.forward_images(x.float().to(cuda))
    for i in range(2):
        _meets_bar(y[i:i + 1], sd, x[i:i + 1], training=True)
    _running_meets_bar(_cpu(m.state_dict()), sd, x, joint=False)


@pytest.mark.parametrize("out_ch", [1, 3, 64, 65, 200])
def test_out_channels(cuda, out_ch):
    """The last product (CHW epilogue, its bias, never split) at widths below, at and above one 64-column tile, and partial
    128-column tiles; training and eval."""
    _, base = _model(cuda, recipe=1)
    g = torch.Generator().manual_seed(out_ch)
    sd = dict(base)
    sd["decoder.conv0.weight"] = torch.randn(out_ch, 128, 1, 1, generator=g) * (2.0 / 128) ** 0.5
    sd["decoder.conv0.bias"] = torch.rand(out_ch, generator=g) - 0.5
    nbytes = _lib.lib().pcrcg_res50unet_arena_bytes(out_ch)
    assert nbytes == 4 * (sum(v.numel() for v in sd.values() if v.dim() == 4) + out_ch + 64 * 13)
    x = _image(15, 1, 72, 88)
    for training in (True, False):
        m = _load(cuda, sd, out_ch, training)
        y = m(x.float().to(cuda))
        assert y.shape == (1, out_ch, 36, 44)
        _meets_bar(y, sd, x, training=training)


@pytest.mark.parametrize("h,w,n", [(1, 1, 2), (1, 7, 1), (3, 5, 2)])
def test_eval_tiny_maps(cuda, h, w, n):
    """Eval mode at 1 x 1, 1 x 7, 3 x 5: 1-pixel maps at every level; the resize with H == 1 and OH == 1."""
    _, sd = _model(cuda, recipe=1)
    x = _image(16, n, h, w)
    y = _load(cuda, sd, training=False)(x.float().to(cuda))
    assert y.shape == (n, 128, *resunet.output_size(h, w))
    _meets_bar(y, sd, x, training=False)


@pytest.mark.parametrize("h,w,n,joint", [
    (1, 1, 2, True),        # the smallest admitted: two images of 1 pixel, every statistic over 2 values
    (17, 33, 2, False),     # per image, layer4 1 x 2: exactly 2 values
    (4, 128, 3, False),     # stem map 2 x 64: 128 rows per image, one full row tile
    (6, 86, 3, False),      # stem map 3 x 43: 129 rows per image, a second row tile of one row
    (8, 400, 2, True),      # aspect ratio 50
])
def test_training_shapes(cuda, h, w, n, joint):
    """The shape rules' edges in training mode.  Where layer4's segments hold 2 values the buffers are held to the pooled
    bar (see _running_meets_bar)."""
    _, sd = _model(cuda, recipe=1)
    x = _image(17, n, h, w)
    m = _load(cuda, sd)
    xd = x.float().to(cuda)
    y = m(xd) if joint else m.forward_images(xd)
    assert y.shape == (n, 128, *resunet.output_size(h, w))
    if joint:
        _meets_bar(y, sd, x, training=True)
    else:
        for i in range(n):
            _meets_bar(y[i:i + 1], sd, x[i:i + 1], training=True)
    _running_meets_bar(_cpu(m.state_dict()), sd, x, joint, pooled=h <= 32 and w <= 64)


def test_odd_full_size_per_image(cuda):
    m, sd = _model(cuda)
    x = _image(18, 1, 241, 321)
    y = m.forward_images(x.float().to(cuda))
    assert y.shape == (1, 128, 122, 162)
    _meets_bar(y, sd, x, training=True)


@pytest.mark.parametrize("h,w,n,joint", [(32, 32, 1, True), (32, 32, 2, False), (1, 32, 3, False)])
def test_statistics_minimum_refused_before_any_launch(cuda, h, w, n, joint):
    """One shape past the statistics limit (layer4 leaves 1 value per segment): PCRCG_EBADARG, and nothing written."""
    m, _ = _model(cuda, recipe=1)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = _image(19, n, h, w).float().to(cuda)
    with pytest.raises(RuntimeError, match=r"code -1\)"):
        m(x) if joint else m.forward_images(x)
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    # the same shape with one more image (joint) or in eval mode runs
    m.eval()
    _meets_bar(m(x), {k: v.cpu() for k, v in before.items()}, x.double().cpu(), training=False)


def test_five_images_per_image_updates(cuda):
    m, sd = _model(cuda, recipe=1)
    x = _image(20, 5, 72, 88)
    y5 = m.forward_images(x.float().to(cuda))
    _running_meets_bar(_cpu(m.state_dict()), sd, x, joint=False)
    m1, _ = _model(cuda, recipe=1)
    singles = torch.cat([m1.forward_images(x[i:i + 1].float().to(cuda)) for i in range(5)])
    assert (singles - y5).abs().max().item() <= 1e-6 * y5.abs().max().item()
    after5 = m.state_dict()
    for k, v in m1.state_dict().items():
        if "running" in k:
            assert (v - after5[k]).abs().max().item() <= 1e-6 * max(1.0, v.abs().max().item()), k
        elif k.endswith("num_batches_tracked"):
            assert torch.equal(v, after5[k]), k
    for i in range(5):
        _meets_bar(y5[i:i + 1], sd, x[i:i + 1], training=True)


def test_state_written_only_where_promised(cuda):
    """eval: nothing but the output.  training: the running buffers and counts, never a parameter."""
    m, _ = _model(cuda, recipe=1)
    x = _image(21, 2, 72, 88).float().to(cuda)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert len(before) == resunet.N_TENSORS
    m.eval()
    m(x)
    m.forward_images(x)
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    m.train()
    m.forward_images(x)
    torch.cuda.synchronize()
    params = {k for k, _ in m.named_parameters()}
    changed = set()
    for k, v in m.state_dict().items():
        if k in params:
            assert torch.equal(v, before[k]), k
        elif not torch.equal(v, before[k]):
            changed.add(k)
    buffers = {k for k, _ in m.named_buffers()}
    assert changed == buffers                                     # every running buffer and count moved, nothing else
    assert all(k.rsplit(".", 1)[1] in ("running_mean", "running_var", "num_batches_tracked") for k in buffers)


def _debug(spec):
    _lib.check(_lib.lib().pcrcg_debug_set(spec.encode() if spec is not None else None), "pcrcg_debug_set")


def test_deterministic_forward_images_bit_identical(cuda):
    """deterministic=1: three per-image training calls, each from an identical copy of the starting state, on images whose
    mean dwarfs their spread (where summation order shows most): bit-identical outputs and running buffers; each within the
    float64 bar; and within summation-order distance of the default path."""
    m, sd = _model(cuda, recipe=1)
    x = _offset_image(22, 4, 72, 88)
    xd = x.float().to(cuda)
    start = {k: v.to(cuda) for k, v in sd.items()}

    def run():
        m.load_state_dict(start)
        y = m.forward_images(xd)
        torch.cuda.synchronize()
        return y, {k: v.detach().clone() for k, v in m.state_dict().items()}
    default = run()
    try:
        _debug("deterministic=1")
        runs = [run() for _ in range(3)]
    finally:
        _debug(None)
        _lib.check(_lib.lib().pcrcg_debug_release(), "pcrcg_debug_release")
    for y, state in runs[1:]:
        assert torch.equal(y, runs[0][0])
        for k, v in state.items():
            assert torch.equal(v, runs[0][1][k]), k
    y, state = runs[0]
    for i in range(4):
        _meets_bar(y[i:i + 1], sd, x[i:i + 1], training=True)
    _running_meets_bar(_cpu(state), sd, x, joint=False)
    d = float((y.double() - default[0].double()).abs().max() / default[0].double().abs().max())
    assert d < 1e-5, d
    for k, v in state.items():
        if "running" in k:
            want = default[1][k].double()
            assert float((v.double() - want).abs().max() / max(1.0, want.abs().max().item())) < 1e-5, k
