"""MI355X replacement for the reference extension module ``grid_subsampling``
(zip:cpp_subsampling/wrapper.cpp:28-33: methods ``subsample`` and ``subsample_batch``).

The points-only form is the one on the hot path (ref:datasets/dataloader.py:18-24).  The reference's optional
``features=`` (float32 [N, d]: the mean of each cell's rows) and ``classes=`` (int32 [N] or [N, d]: each cell's most
frequent label) are carried through the same grid by ops.grid_subsample_ex and come back in the barycentres' row order,
bit for bit what the reference returns.  Two inputs on which the reference is undefined:

* ``subsample_batch`` with 2-D classes of more than one column and more than one cloud raises RuntimeError: the
  reference slices a cloud's labels with an end that is out of range there (grid_subsampling.cpp:155-156), so there is
  nothing to reproduce.  One cloud, or one label column, is exact.
* a cloud of length 0 yields length 0 and no rows, as in the points-only form (the reference divides by zero)."""
import numpy as np
import torch

from ... import ops
from .._common import as_tensor, to_device

_METHODS = ("barycenters", "voxelcenters")
_BAD_METHOD = 'Error parsing method. Valid method names are "barycenters" and "voxelcenters" '
_BAD_FEATURES = "Wrong dimensions : features.shape is not (N, d)"
_BAD_CLASSES = "Wrong dimensions : classes.shape is not (N,) or (N, d)"


def _inputs(points, features, classes):
    """The conversions and shape checks of wrapper.cpp:106-224 / :380-468, in its order, before the device is touched:
    -> (points, features or None, classes or None, was_numpy)"""
    p, was_numpy = as_tensor(points, torch.float32, "Error converting input points to numpy arrays of type float32")
    f = c = None
    if features is not None:
        f, _ = as_tensor(features, torch.float32, "Error converting input features to numpy arrays of type float32")
    if classes is not None:
        c, _ = as_tensor(classes, torch.int32, "Error converting input classes to numpy arrays of type int32")
    return p, f, c, was_numpy


def _check_extras(p, f, c):
    if f is not None and f.dim() != 2:
        raise RuntimeError(_BAD_FEATURES)
    if c is not None and c.dim() not in (1, 2):
        raise RuntimeError(_BAD_CLASSES)
    if f is not None and f.shape[0] != p.shape[0]:
        raise RuntimeError(_BAD_FEATURES)
    if c is not None and c.shape[0] != p.shape[0]:
        raise RuntimeError(_BAD_CLASSES)


def _extras(f, c, sub_f, sub_c, was_numpy):
    out = [t for t, given in ((sub_f, f), (sub_c, c)) if given is not None]
    return [t.cpu().numpy() for t in out] if was_numpy else out


def subsample_batch(points, batches, *, features=None, classes=None, sampleDl=0.1, method="barycenters", max_p=0,
                    verbose=0):
    """(points f32 [N,3], batches i32 [B]) -> (sub_points f32 [M,3], sub_batches i32 [B]); with ``features`` f32 [N,d]
    and / or ``classes`` i32 [N] or [N,d] the tuple continues with sub_features f32 [M,d] and / or sub_classes i32 [M,d]
    ([M,1] for 1-D classes), in this order (zip:cpp_subsampling/wrapper.cpp:62-330).  numpy in -> numpy out; device
    tensors in -> device tensors out."""
    if method not in _METHODS:  # wrapper.cpp:92-96
        raise RuntimeError(_BAD_METHOD)
    p, f, c, was_numpy = _inputs(points, features, classes)
    b, _ = as_tensor(batches, torch.int32, "Error converting input batches to numpy arrays of type int32")
    if p.dim() != 2 or p.shape[1] != 3:
        raise RuntimeError("Wrong dimensions : points.shape is not (N, 3)")
    if b.dim() > 1:
        raise RuntimeError("Wrong dimensions : batches.shape is not (B,) ")
    _check_extras(p, f, c)
    if f is None and c is None:
        sub, sub_len = ops.grid_subsample(to_device(p), to_device(b), float(sampleDl), int(max_p))
        extras = []
    else:
        if c is not None and c.dim() == 2 and c.shape[1] > 1 and b.numel() > 1:
            raise RuntimeError("pcrcg_amd: subsample_batch with classes of more than one column and more than one cloud is "
                               "undefined in the reference (it slices the labels of every cloud after the first out of "
                               "range, grid_subsampling.cpp:155-156); pass one cloud or one label column")
        sub, sub_len, sub_f, sub_c = ops.grid_subsample_ex(to_device(p), to_device(b), float(sampleDl), int(max_p),
                                                           None if f is None else f.to("cuda"),
                                                           None if c is None else to_device(c))
        extras = _extras(f, c, sub_f, sub_c, was_numpy)
    if sub.shape[0] < 1:  # wrapper.cpp:266-270
        raise RuntimeError("Error")
    if was_numpy:
        sub, sub_len = sub.cpu().numpy(), sub_len.cpu().numpy()
    return (sub, sub_len, *extras)


def subsample(points, *, features=None, classes=None, sampleDl=0.1, method="barycenters", verbose=0):
    """Single-cloud variant (zip:cpp_subsampling/wrapper.cpp:338-565): returns the sub-sampled points, or with
    ``features`` and / or ``classes`` the tuple (sub_points[, sub_features][, sub_classes])."""
    if method not in _METHODS:
        raise RuntimeError(_BAD_METHOD)
    p, f, c, was_numpy = _inputs(points, features, classes)
    if p.dim() != 2 or p.shape[1] != 3:
        raise RuntimeError("Wrong dimensions : points.shape is not (N, 3)")
    _check_extras(p, f, c)
    p = to_device(p)
    b = torch.tensor([p.shape[0]], dtype=torch.int32, device=p.device)
    if f is None and c is None:
        sub, _ = ops.grid_subsample(p, b, float(sampleDl), 0)
        extras = []
    else:
        sub, _, sub_f, sub_c = ops.grid_subsample_ex(p, b, float(sampleDl), 0, None if f is None else f.to("cuda"),
                                                     None if c is None else to_device(c))
        extras = _extras(f, c, sub_f, sub_c, was_numpy)
    if sub.shape[0] < 1:
        raise RuntimeError("Error")
    if was_numpy:
        sub = sub.cpu().numpy()
    return (sub, *extras) if extras else sub
