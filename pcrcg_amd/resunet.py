"""PCR-CG's 2-D image backbone, Res50UNet (ref:models/resunet.py:163-188), on the HIP path of csrc/conv2d.hip.

The module tree, parameter and buffer names and shapes are the reference's (encoder.conv1.weight, encoder.layer1.0.
downsample.1.running_var, ..., decoder.up4.bn1_2.*, decoder.conv0.bias), and so is the initialisation, which consumes the
RNG in the same order: default init as the modules are built, then normal_(0, sqrt(2 / (k k cout))) over the ResNet's
convolutions and gamma = 1 / beta = 0, then the decoder's default init.  A checkpoint of the reference loads as it is.

forward(x [B, 3, H, W]) follows torch's semantics: training mode normalises with the batch's statistics (and updates the
running buffers), .eval() with the running statistics.  forward_images(x [n, 3, H, W]) runs n independent batches of one
in one call -- what PCR-CG does, one image at a time (ref:models/architectures.py:278-281) -- with the running statistics
updated in image order.  The reference never trains the backbone (it detaches what it gathers), so there is no backward:
outputs carry no grad_fn.
"""
import ctypes

import torch
from torch import nn

from . import _lib

_PLANES, _BLOCKS, _STRIDES = (64, 128, 256, 512), (3, 4, 6, 3), (1, 2, 2, 2)
N_TENSORS = 392


class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample


class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inplanes = 64
        for i, (planes, blocks, stride) in enumerate(zip(_PLANES, _BLOCKS, _STRIDES)):
            # the downsample branch is built before its block (RNG order)
            down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                                 nn.BatchNorm2d(planes * 4))
            layer = [_Bottleneck(inplanes, planes, stride, down)]
            inplanes = planes * 4
            layer += [_Bottleneck(inplanes, planes, 1, None) for _ in range(1, blocks)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*layer))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, (2.0 / n) ** 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()


class _UpProjection(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, kernel_size=5, stride=1, padding=2, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv1_2 = nn.Conv2d(cout, cout, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1_2 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cin, cout, kernel_size=5, stride=1, padding=2, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)


class _Decoder(nn.Module):
    def __init__(self, output_channel):
        super().__init__()
        f = 2048
        for i in range(4):
            setattr(self, f"up{i + 1}", _UpProjection(f, f // 2))
            f //= 2
        self.conv0 = nn.Conv2d(f, output_channel, kernel_size=1, stride=1, padding=0, bias=True)


def output_size(h, w):
    """(H, W) of the feature map for an h x w image: twice the size after the stem (ceil h/2) and the max-pool (ceil)."""
    return 2 * (((h + 1) // 2 + 1) // 2), 2 * (((w + 1) // 2 + 1) // 2)


class Res50UNet(nn.Module):
    """ref:models/resunet.py Res50UNet(output_channel, pretrained) on csrc/conv2d.hip."""

    def __init__(self, output_channel=128, pretrained=False):
        super().__init__()
        if pretrained is not False:
            raise ValueError("pcrcg_amd.resunet.Res50UNet: pretrained weights are a download (ImageNet / MoCo / SimCLR / "
                             "SwAV); build with pretrained=False and load a checkpoint (pcrcg_amd.resunet.load_checkpoint)")
        self.output_channel = int(output_channel)
        self.encoder = _Encoder()
        self.decoder = _Decoder(self.output_channel)
        self._arena = None            # (key, arena tensor)
        self._table = None            # (key, ctypes pointer array)
        self._ws = {}                 # device -> workspace tensor

    # ---- the derived weights (repacked when a tensor moves or a parameter's _version changes) --------------------------
    def _tensors(self):
        ts = list(self.state_dict(keep_vars=True).values())
        if len(ts) != N_TENSORS:
            raise RuntimeError(f"pcrcg_amd.Res50UNet: {len(ts)} state tensors, expected {N_TENSORS}")
        return ts

    def _state_table(self, ts):
        key = tuple(t.data_ptr() for t in ts)
        if self._table is None or self._table[0] != key:
            self._table = (key, (ctypes.c_void_p * N_TENSORS)(*key))
        return self._table[1]

    def _packed(self, ts, table, stream):
        key = tuple((t.data_ptr(), t._version) for t in self.parameters())
        if self._arena is None or self._arena[0] != key:
            L = _lib.lib()
            nbytes = L.pcrcg_res50unet_arena_bytes(self.output_channel)
            arena = torch.empty(nbytes // 4, dtype=torch.float32, device=ts[0].device)
            _lib.check(L.pcrcg_res50unet_pack(table, N_TENSORS, self.output_channel, ctypes.c_void_p(arena.data_ptr()),
                                              ctypes.c_void_p(stream)), "pcrcg_res50unet_pack")
            self._arena = (key, arena)
        return self._arena[1]

    def _load_from_state_dict(self, *args, **kwargs):
        self._arena = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _run(self, x, joint):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"pcrcg_amd.Res50UNet: input must be [B, 3, H, W], got {tuple(x.shape)}")
        ts = self._tensors()
        dev = ts[0].device
        if dev.type != "cuda":
            raise RuntimeError("pcrcg_amd.Res50UNet runs on the GPU only (HIP kernels): move the module with .cuda()")
        for t in ts:
            if t.device != dev or not t.is_contiguous() or (t.dtype != torch.float32 and t.dtype != torch.int64):
                raise RuntimeError("pcrcg_amd.Res50UNet: every parameter and buffer must be a contiguous fp32 (counts: int64) "
                                   "tensor on one device")
        n, _, h, w = x.shape
        x = x.detach().to(dev, torch.float32).contiguous()
        stream = torch.cuda.current_stream(dev).cuda_stream
        table = self._state_table(ts)
        arena = self._packed(ts, table, stream)
        L = _lib.lib()
        ws_bytes = L.pcrcg_res50unet_ws_bytes(n, h, w)
        if ws_bytes == 0:
            raise ValueError(f"pcrcg_amd.Res50UNet: unsupported input shape {tuple(x.shape)}")
        ws = self._ws.get(dev)
        if ws is None or ws.numel() < ws_bytes:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            self._ws[dev] = ws
        oh, ow = output_size(h, w)
        out = torch.empty((n, self.output_channel, oh, ow), dtype=torch.float32, device=dev)
        _lib.check(L.pcrcg_res50unet_forward(ctypes.c_void_p(arena.data_ptr()), table, N_TENSORS, self.output_channel,
                                             ctypes.c_void_p(x.data_ptr()), n, h, w, int(joint), int(self.training),
                                             ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws_bytes,
                                             ctypes.c_void_p(stream)), "pcrcg_res50unet_forward")
        return out

    def forward(self, x):
        """torch's semantics: training mode -> statistics over the whole batch; eval -> running statistics."""
        return self._run(x, joint=True)

    def forward_images(self, x):
        """n independent batch-of-one runs in one call (training mode: per-image statistics, running buffers updated in
        image order, num_batches_tracked += n); in eval mode the same as forward."""
        return self._run(x, joint=False)


def build_backbone(name, nclasses, pretrained=False):
    """ref:models/__init__.py build_backbone for the backbone PCR-CG ships (image_feature: Res50UNet(128))."""
    if name != "Res50UNet":
        raise NotImplementedError(f"pcrcg_amd.resunet.build_backbone: {name!r} is not implemented; supported: 'Res50UNet'")
    return Res50UNet(nclasses, pretrained=pretrained)


def load_checkpoint(model, path):
    """ref:lib/trainer.py:14-21,114-128 (Trainer.resume_checkpoint + load_state_with_same_shape) for the 2-D backbone: the
    checkpoint's state['model'] with the first 9 characters of every key dropped ('backbone.'), only names that exist in
    `model` with the same shape, loaded with strict=False.  Returns the names that were loaded."""
    state = torch.load(path, map_location="cpu")
    own = model.state_dict()
    kept = {}
    for k, v in state["model"].items():
        k = k[9:]
        if k in own and tuple(own[k].shape) == tuple(v.shape):
            kept[k] = v
    model.load_state_dict(kept, strict=False)
    return sorted(kept)
