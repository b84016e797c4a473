"""Ragged-batch marshalling shared by the registration back end and its siblings (registration, modelnet, modelnet_prep,
kitti, tester): lists of per-item arrays in, the concatenated device tensors, offsets, chunk lists and cell grids the
batched library entries take out.  Plain functions; each rule lives here once.  Nothing here picks a device: every
function that touches one is handed `dev`, so a caller's host checks all run before its device lookup.
"""
import numpy as np
import torch

from . import _lib

MAX_BATCH = 65535         # items per batched library call (include/pcrcg.h)
MAX_ROWS = 0x7FFFFFFF     # concatenated rows per call: the entries index rows with an int
READS = [0]               # device -> host reads made through `read` (registration.D2H_READS)


def read(t):
    """The counted way to the host."""
    READS[0] += 1
    return t.cpu().numpy()


def device(xs, module):
    """The device of the first HIP tensor among xs, else the current one."""
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise RuntimeError(f"pcrcg_amd.{module}: no HIP device is visible (there is no CPU implementation)")
    return torch.device("cuda", torch.cuda.current_device())


def shape_of(x):
    """The shape of a tensor, an array or a nested list (nothing is copied)."""
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def rows(x):
    return x.shape[0] if hasattr(x, "shape") else len(x)


def tensors(xs):
    return [x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)) for x in xs]


def join(ts, dev, dtype, part=lambda t: t):
    """Tensors (each through `part`) -> one contiguous device tensor of `dtype`: when all are on the host they are joined
    there and travel in ONE upload, otherwise each is converted on the device and joined there."""
    if all(not t.is_cuda for t in ts):
        return torch.cat([part(t).to(dtype) for t in ts]).to(dev).contiguous()
    return torch.cat([part(t).to(device=dev, dtype=dtype) for t in ts]).contiguous()


def upload(xs, dev, dtype, cols=None, name="arrays"):
    """Per-item [N_b, cols] arrays (numpy, CPU or HIP tensors) -> one [sum N_b, cols] device tensor (`join`'s rule)."""
    t = join(tensors(xs), dev, dtype)
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{name} must be [N, {cols or 'C'}] arrays, got {tuple(t.shape)} concatenated")
    return t


def upload_f64(x, dev):
    """One array of parameters (viewpoints, start transforms) -> a contiguous float64 device tensor."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float64))
    return t.to(device=dev, dtype=torch.float64).contiguous()


def chunks(B, per_call, cap, who, *row_lists):
    """[(b0, b1) ...]: B items in runs of min(per_call (None: all), cap); no run may hold more than MAX_ROWS rows of any
    of the row_lists (per-item row counts)."""
    P = max(1, min(B if per_call is None else int(per_call), B, cap))
    out = [(b0, min(B, b0 + P)) for b0 in range(0, B, P)]
    if any(sum(ns[b0:b1]) > MAX_ROWS for ns in row_lists for b0, b1 in out):
        raise ValueError(f"{who}: more than 2^31 - 1 rows per call; lower pairs_per_call")
    return out


def per_call_within(budget, per_item_bytes):
    """The default items per call: as many as keep a workspace of per_item_bytes each within budget."""
    return max(1, budget // max(per_item_bytes, 1))


def offsets(dev, *lists, lengths=()):
    """ONE int32 upload -> views of it: the [nb + 1] prefix sums of every list, then every list of `lengths` as it is."""
    parts = [np.cumsum([0] + list(ns)) for ns in lists] + [np.asarray(ns, dtype=np.int64) for ns in lengths]
    if len(parts) == 1:
        return (torch.tensor(parts[0], dtype=torch.int32, device=dev),)
    return torch.tensor(np.concatenate(parts), dtype=torch.int32, device=dev).split([len(p) for p in parts])


def cell_grid(pts, n_tot, lengths, nb, cell, stream):
    """pcrcg_cellgrid_build over nb concatenated clouds (pts [n_tot,3] float32, lengths [nb] int32, both on the device) ->
    the grid tensor.  An empty stack is passed as a null pointer."""
    L = _lib.lib()
    gbytes = L.pcrcg_cellgrid_ws_bytes(n_tot, nb)
    grid = torch.empty(gbytes, dtype=torch.uint8, device=pts.device)
    _lib.check(L.pcrcg_cellgrid_build(pts.data_ptr() if n_tot else None, n_tot, lengths.data_ptr(), nb, cell, grid.data_ptr(),
                                      gbytes, stream), "pcrcg_cellgrid_build")
    return grid


def check_viewpoints(viewpoints, B, who):
    if viewpoints is not None and shape_of(viewpoints) != (B, 3):
        raise ValueError(f"{who}: viewpoints must be [{B}, 3] (one per cloud), got shape {shape_of(viewpoints)}")


def lift(x, shape, what):
    """A single item's optional argument of `shape` -> the batch-of-one form (None stays None)."""
    if x is None:
        return None
    if shape_of(x) != shape:
        raise ValueError(f"{what}, got shape {shape_of(x)}")
    return x[None] if isinstance(x, (torch.Tensor, np.ndarray)) else np.asarray(x, dtype=np.float64)[None]


def descriptor_width(who, b, fs, ft, n, m, c):
    """Pair b's descriptors: one row per point, and the batch's one width c (None: this pair sets it) -> c."""
    if rows(fs) != n or rows(ft) != m:
        raise ValueError(f"{who}: pair {b}: the descriptors must have one row per point")
    cb = (fs.shape[1], ft.shape[1])
    if c is None:
        c = cb[0]
    if cb != (c, c):
        raise ValueError(f"{who}: pair {b}: descriptor width {cb}, the batch uses {c}")
    return c


def seed_list(seeds, n, who, items, bits=24, plural="seeds", one="seed"):
    """An int (every item) or n ints in [0, 2^bits) -> the list of n."""
    seeds = [int(seeds)] * n if np.ndim(seeds) == 0 else [int(x) for x in seeds]
    if len(seeds) != n:
        raise ValueError(f"{who}: {len(seeds)} {plural} for {n} {items}")
    if any(not 0 <= x < (1 << bits) for x in seeds):
        raise ValueError(f"{who}: every {one} must lie in [0, 2^{bits})")
    return seeds
