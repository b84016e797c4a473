"""Ground-truth correspondences on the device (mirror of get_correspondences,
ref:lib/benchmark_utils.py:121-134, which loops over the source points in Python and asks an open3d
KD-tree for the target points within `search_voxel_size` of each).

Same result contract: an int64 [K,2] tensor of (src index, tgt index), source-major, the targets of one
source point ordered by increasing distance (FLANN returns radius-search hits sorted), optionally the K
nearest only.  open3d holds points and the 4x4 transform in float64, so membership `d < radius` is decided in
float64 here too: the cell grid of the hot path's radius search (fp32, built with a slightly inflated radius)
supplies the candidates, and the kernel re-measures every candidate in float64 from the float64-moved source point,
ranks the hits by (distance, target index) and writes them out (csrc/radius.hip: k_correspond_rows / _emit).  Two
launches and one scan; the host reads two integers (longest list, number of pairs) to size the result.
Equal distances are ordered by target index.

`get_correspondences_batch` is the same for B pairs in one call: ONE cell grid over all targets with a hash table per
pair, the same two launches and scan over the concatenated source rows (k_correspond_rows_batch / _emit_batch), and one
read-back per attempt of B + 1 integers (longest list, pairs per pair)."""
import ctypes

import numpy as np
import torch

from . import _lib, ops

_INFLATE = 1.0 + 1e-4     # fp32 candidate radius: never loses a pair that is inside in float64
_ROW_CAP = 1024           # hits one source point can stage (csrc/radius.hip kCorrCap)


def get_correspondences(src_pcd, tgt_pcd, trans, search_voxel_size, K=None):
    """src_pcd [N,3], tgt_pcd [M,3] float32 device tensors, trans [4,4] (any float dtype, host or device)."""
    if not (isinstance(src_pcd, torch.Tensor) and src_pcd.is_cuda and tgt_pcd.is_cuda):
        raise RuntimeError("pcrcg_amd.get_correspondences: point clouds must be tensors on a HIP device")
    dev = src_pcd.device
    n, m = src_pcd.shape[0], tgt_pcd.shape[0]
    if n == 0 or m == 0:
        return torch.empty((0, 2), dtype=torch.int64, device=dev)
    L = _lib.lib()
    t64 = np.ascontiguousarray(torch.as_tensor(trans, dtype=torch.float64).cpu().numpy().reshape(4, 4))
    src = src_pcd.float().contiguous()
    radius = float(search_voxel_size)
    grid = ops.CellGrid(tgt_pcd.float().contiguous(), torch.tensor([m], dtype=torch.int32, device=dev), radius * _INFLATE)
    keep = int(K) if K is not None else 0
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    cols = 32
    while True:
        stage = torch.empty((n, cols), dtype=torch.int32, device=dev)
        head = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.pcrcg_correspondences_rows(src.data_ptr(), n, t64.ctypes.data_as(ctypes.c_void_p), radius, keep, m,
                                                grid.grid.data_ptr(), cols, stage.data_ptr(), counts.data_ptr(),
                                                head.data_ptr(), stream), "pcrcg_correspondences_rows")
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        longest, total = (int(v) for v in torch.stack([head[0].to(torch.int64), ends[-1]]).tolist())   # ONE read-back
        if longest > _ROW_CAP:
            raise RuntimeError(f"pcrcg_amd.get_correspondences: a source point has {longest} targets within the radius "
                               f"(more than the {_ROW_CAP} a row can stage)")
        need = min(longest, keep) if keep else longest
        if need <= cols:
            break
        cols = need
    out = torch.empty((total, 2), dtype=torch.int64, device=dev)
    if total:
        offsets = ends - counts
        _lib.check(L.pcrcg_correspondences_emit(stage.data_ptr(), cols, counts.data_ptr(), offsets.data_ptr(), n,
                                                out.data_ptr(), stream), "pcrcg_correspondences_emit")
    return out


_MAX_BATCH = 65535        # pcrcg_correspondences_batch_rows: B


def get_correspondences_batch(src_list, tgt_list, transforms, radius, K=None):
    """get_correspondences for B pairs in one call -> a list of B [K_b, 2] int64 device tensors, pair b's equal to
    get_correspondences(src_list[b], tgt_list[b], transforms[b], radius, K): indices local to the pair, source-major,
    the targets of a source point by (float64 distance, target index).  src_list[b] [N_b,3], tgt_list[b] [M_b,3]: float32
    device tensors; transforms: B [4,4] transforms (a list, or a [B,4,4] array or tensor, host or device); one radius and
    one K for all pairs.  A pair with an empty side gives [0, 2].

    One cell grid over all targets (nb = B: a source point only ever sees targets of its own pair), two launches and one
    scan per attempt, and ONE read-back per attempt: the longest row and the B pair counts.  As for one pair, the rows are
    run again with wider staging when the longest row exceeds it, and a row of more than 1024 hits raises."""
    src_list, tgt_list = list(src_list), list(tgt_list)
    B = len(src_list)
    if B == 0:
        raise ValueError("get_correspondences_batch: no pairs")
    if B > _MAX_BATCH:
        raise ValueError(f"get_correspondences_batch: {B} pairs in one call, at most {_MAX_BATCH}")
    if len(tgt_list) != B or len(transforms) != B:
        raise ValueError(f"get_correspondences_batch: list lengths differ ({B}, {len(tgt_list)}, {len(transforms)})")
    for x in src_list + tgt_list:
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise RuntimeError("pcrcg_amd.get_correspondences_batch: point clouds must be tensors on a HIP device")
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError(f"get_correspondences_batch: a cloud must be [N, 3], got {tuple(x.shape)}")
    dev = src_list[0].device
    ns, ms = [int(x.shape[0]) for x in src_list], [int(x.shape[0]) for x in tgt_list]
    # a pair with an empty side has no correspondences: its sources are left out, so no row is spent on it
    ns_run = [n if m else 0 for n, m in zip(ns, ms)]
    n_total, m_total = sum(ns_run), sum(ms)
    empty = torch.empty((0, 2), dtype=torch.int64, device=dev)
    if n_total == 0:
        return [empty.clone() for _ in range(B)]
    L = _lib.lib()
    if isinstance(transforms, torch.Tensor):
        t64 = transforms.to(device=dev, dtype=torch.float64).reshape(B, 16).contiguous()
    else:
        t64 = torch.from_numpy(np.stack([np.asarray(torch.as_tensor(t, dtype=torch.float64).cpu().numpy()).reshape(16)
                                         for t in transforms])).to(dev)
    src = torch.cat([x.float() for x, n in zip(src_list, ns_run) if n], 0).contiguous()
    tgt = torch.cat([x.float() for x in tgt_list], 0).contiguous()
    src_off = torch.tensor(np.cumsum([0] + ns_run), dtype=torch.int32, device=dev)
    radius = float(radius)
    grid = ops.CellGrid(tgt, torch.tensor(ms, dtype=torch.int32, device=dev), radius * _INFLATE)
    keep = int(K) if K is not None else 0
    counts = torch.empty(n_total, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    off64 = src_off.long()
    cols = 32
    while True:
        stage = torch.empty((n_total, cols), dtype=torch.int32, device=dev)
        head = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.pcrcg_correspondences_batch_rows(src.data_ptr(), src_off.data_ptr(), n_total, B, t64.data_ptr(), radius,
                                                      keep, m_total, grid.grid.data_ptr(), cols, stage.data_ptr(),
                                                      counts.data_ptr(), head.data_ptr(), stream),
                   "pcrcg_correspondences_batch_rows")
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        bounds = torch.cat([ends.new_zeros(1), ends])[off64]                 # pairs before each pair's first row
        small = torch.cat([head.to(torch.int64), bounds[1:] - bounds[:-1]]).tolist()      # ONE read-back
        longest, per_pair = small[0], small[1:]
        if longest > _ROW_CAP:
            raise RuntimeError(f"pcrcg_amd.get_correspondences_batch: a source point has {longest} targets within the "
                               f"radius (more than the {_ROW_CAP} a row can stage)")
        need = min(longest, keep) if keep else longest
        if need <= cols:
            break
        cols = need
    total = sum(per_pair)
    out = torch.empty((total, 2), dtype=torch.int64, device=dev)
    if total:
        offsets = ends - counts
        _lib.check(L.pcrcg_correspondences_batch_emit(stage.data_ptr(), cols, counts.data_ptr(), offsets.data_ptr(),
                                                      src_off.data_ptr(), n_total, B, out.data_ptr(), stream),
                   "pcrcg_correspondences_batch_emit")
    return list(out.split(per_pair))
