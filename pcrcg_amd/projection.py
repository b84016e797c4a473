"""PCR-CG's RGB-D projection and SuperGlue valid maps on the device (pcrcg_project_depth, pcrcg_superglue_valid_maps).

`Projection` is a drop-in for the reference's (ref:projection.py): same constructor, same `projection(points, depth_map,
world2camera)` signature and results -- bit for bit, including the reference's rounding -- on
device tensors.  `superglue_valid_maps` paints the two valid maps of one image pair the way the data loader does
(ref:datasets/indoor.py:284-299).  A loader that hands raw frames to KPFCNN / PairStreams needs neither:
the fused pcrcg_inject_frames projects inside the input build."""
import ctypes

import torch

from . import _lib
from .ops import _dev, _ptr, _stream, _ws, matrix16

_F32, _I64 = torch.float32, torch.int64


class Projection(object):
    def __init__(self, intrinsic_matrix=0, thresh=0.1):
        """intrinsic_matrix: 4x4 (or 3x3) torch.FloatTensor, as the reference takes it."""
        self.intrinsics = intrinsic_matrix
        self.thresh = thresh

    def projection(self, points, depth_map, world2camera):
        """points [n, 3] f32 and depth_map [H, W] (or [1, H, W]) f32 on the device; world2camera 4x4.
        -> inds2d [k, 2] i64 (column, row), inds3d [k] i64 (ascending point index), on the device.  The count is read
        back once, to size the outputs."""
        L = _lib.lib()
        pts = _dev(points, _F32, "points").contiguous()
        depth = _dev(depth_map, _F32, "depth_map").squeeze(0).contiguous()
        if pts.dim() != 2 or pts.shape[1] != 3 or depth.dim() != 2:
            raise RuntimeError("pcrcg_amd.Projection: points must be [n, 3] and depth_map [H, W]")
        n, dev = int(pts.shape[0]), pts.device
        h, w = int(depth.shape[0]), int(depth.shape[1])
        i2 = torch.empty((max(n, 1), 2), dtype=_I64, device=dev)
        i3 = torch.empty(max(n, 1), dtype=_I64, device=dev)
        k = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = L.pcrcg_project_depth_ws_bytes(n)
        ws = _ws.get("project_depth", nbytes, dev)
        _lib.check(L.pcrcg_project_depth(pts.data_ptr(), n, depth.data_ptr(), h, w, matrix16(world2camera),
                                         matrix16(self.intrinsics), float(self.thresh), i2.data_ptr(), i3.data_ptr(),
                                         k.data_ptr(), ws.data_ptr(), nbytes, _stream()), "pcrcg_project_depth")
        kk = int(k.item())
        return i2[:kk], i3[:kk]


def superglue_valid_maps(keypoints0, keypoints1, matches, confidence, window=5, size=(160, 120)):
    """The source and target valid maps of one image pair from SuperGlue's keypoints0 [n0, 2], keypoints1 [n1, 2],
    matches [n0] (-1: unmatched) and match_confidence [n0], all on the device; window = the config's window_size.
    -> (src_valid, tgt_valid), each [size[0], size[1]] f32 (the reference's [160, 120]: first index the column x)."""
    L = _lib.lib()
    kp0 = _dev(keypoints0.to(_F32), _F32, "keypoints0").contiguous()
    kp1 = _dev(keypoints1.to(_F32), _F32, "keypoints1").contiguous()
    m = _dev(matches.to(_I64), _I64, "matches").contiguous()
    conf = _dev(confidence.to(_F32), _F32, "confidence").contiguous()
    if kp0.dim() != 2 or kp0.shape[1] != 2 or kp1.dim() != 2 or kp1.shape[1] != 2:
        raise RuntimeError("pcrcg_amd.superglue_valid_maps: keypoints must be [n, 2]")
    n0, n1 = int(kp0.shape[0]), int(kp1.shape[0])
    if m.shape != (n0,) or conf.shape != (n0,):
        raise RuntimeError("pcrcg_amd.superglue_valid_maps: matches and confidence must be [len(keypoints0)]")
    src = torch.empty(size, dtype=_F32, device=kp0.device)
    tgt = torch.empty(size, dtype=_F32, device=kp0.device)
    _lib.check(L.pcrcg_superglue_valid_maps(_ptr(kp0) if n0 else None, n0, _ptr(kp1) if n1 else None, n1,
                                            _ptr(m) if n0 else None, _ptr(conf) if n0 else None, int(window), size[0],
                                            size[1], src.data_ptr(), tgt.data_ptr(), _stream()),
               "pcrcg_superglue_valid_maps")
    return src, tgt
