"""Float64 restatement of PCR-CG's Res50UNet forward (ref:models/resunet.py, ref:models/resnet.py), written from its
semantics: the oracle of tests/test_resunet_*.py.

resunet_forward(sd, x, training, joint) runs the network on the CPU in float64 from a state_dict `sd` (any dtype; taken as
float64).  training=True: BatchNorm2d with batch statistics (biased variance, eps 1e-5) over all images (joint=True, torch's
batch semantics) or over each image on its own (joint=False, PCR-CG's one-image calls); the running statistics that the
call leaves behind (momentum 0.1, unbiased variance; per image in order when joint=False) are returned as a dict.
training=False: the running statistics."""
import torch
import torch.nn.functional as F

PLANES, BLOCKS, STRIDES = (64, 128, 256, 512), (3, 4, 6, 3), (1, 2, 2, 2)
EPS, MOMENTUM = 1e-5, 0.1


def recipe(model, seed=1):
    """Non-trivial BatchNorm state: gamma in [-1.5, 1.5] (negative included), beta in [-0.5, 0.5], running mean in
    [-0.2, 0.2], running variance in [0.5, 2.0]; drawn from a seeded generator in state_dict order."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(torch.rand(c, generator=g) * 3.0 - 1.5)
                m.bias.copy_(torch.rand(c, generator=g) - 0.5)
                m.running_mean.copy_(torch.rand(c, generator=g) * 0.4 - 0.2)
                m.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.5)


class _State:
    def __init__(self, sd, training, joint, dtype):
        self.sd = {k: v.detach().to(dtype) if v.is_floating_point() else v.clone() for k, v in sd.items()}
        self.training, self.joint = training, joint
        self.running = {}

    def conv(self, name, x, stride=1, padding=0, bias=False):
        return F.conv2d(x, self.sd[name + ".weight"], self.sd.get(name + ".bias") if bias else None, stride, padding)

    def bn(self, name, x):
        g, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
        rm, rv = self.sd[name + ".running_mean"].clone(), self.sd[name + ".running_var"].clone()
        if not self.training:
            return (x - rm[None, :, None, None]) / torch.sqrt(rv[None, :, None, None] + EPS) * g[None, :, None, None] \
                + b[None, :, None, None]
        groups = [x] if self.joint else [x[i:i + 1] for i in range(x.shape[0])]
        outs = []
        for xs in groups:
            n = xs.numel() // xs.shape[1]
            mean = xs.mean(dim=(0, 2, 3))
            var = ((xs - mean[None, :, None, None]) ** 2).sum(dim=(0, 2, 3)) / n
            outs.append((xs - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS)
                        * g[None, :, None, None] + b[None, :, None, None])
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
            rv = (1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1)
        self.running[name] = (rm, rv, len(groups))
        return torch.cat(outs)


def resunet_forward(sd, x, training=True, joint=True, dtype=torch.float64):
    """-> (output [n, C, 2 ceil(ceil(h/2)/2), ...], {bn name: (running_mean, running_var, updates)}).  dtype=torch.float32:
    the same network in plain fp32 (the error bar of the GPU tests)."""
    S = _State(sd, training, joint, dtype)
    x = x.to(dtype)
    relu = torch.relu
    x = relu(S.bn("encoder.bn1", S.conv("encoder.conv1", x, 2, 3)))
    x = F.max_pool2d(x, 3, 2, 1)
    feats = []
    for L in range(4):
        for b in range(BLOCKS[L]):
            p = f"encoder.layer{L + 1}.{b}"
            s = STRIDES[L] if b == 0 else 1
            o = relu(S.bn(p + ".bn1", S.conv(p + ".conv1", x)))
            o = relu(S.bn(p + ".bn2", S.conv(p + ".conv2", o, s, 1)))
            o = S.bn(p + ".bn3", S.conv(p + ".conv3", o))
            res = S.bn(p + ".downsample.1", S.conv(p + ".downsample.0", x, s)) if b == 0 else x
            x = relu(o + res)
        feats.append(x)
    x = feats[3]
    for u in range(4):
        p = f"decoder.up{u + 1}"
        size = feats[2 - u].shape[2:] if u < 3 else (feats[0].shape[2] * 2, feats[0].shape[3] * 2)
        x = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)
        c1 = relu(S.bn(p + ".bn1", S.conv(p + ".conv1", x, 1, 2)))
        bran1 = S.bn(p + ".bn1_2", S.conv(p + ".conv1_2", c1, 1, 1))
        bran2 = S.bn(p + ".bn2", S.conv(p + ".conv2", x, 1, 2))
        x = relu(bran1 + bran2)
        if u < 3:
            x = x + feats[2 - u]
    return S.conv("decoder.conv0", x, bias=True), S.running
