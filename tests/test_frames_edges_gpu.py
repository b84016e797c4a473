"""GPU: pcrcg_prepare_frames (csrc/frames.hip) at its edges through the raw entry, bit for bit against the nearest-neighbour
rule restated in tests/indoor_ref.py: up-scaling, one-pixel axes, ratios at which the source index is an exact integer
before the floor, one kind of frame only, outputs of very different areas (the launch grid is sized by the larger), the int16
boundary values of depth, the channel planes of colour, and the argument checks.  Every output buffer is followed by a guard
band that must keep its fill."""
import numpy as np
import pytest
import torch

from pcrcg_amd import _lib

from . import indoor_ref as IR

pytestmark = pytest.mark.gpu

GUARD = 1024
EBADARG = -1        # include/pcrcg.h PCRCG_EBADARG


def _call(cuda, color, csize, depth, dsize, color_null=False, depth_null=False, F=None, G=None, cshape=None, dshape=None):
    """The raw entry on real buffers -> (rc, colour output [F, 3, oh, ow] or None, depth output [G, ohd, owd] or None).  Both
    outputs are pre-filled with NaN and followed by GUARD floats of NaN, which must still be NaN afterwards."""
    L = _lib.lib()
    F = (0 if color is None else color.shape[0]) if F is None else F
    G = (0 if depth is None else depth.shape[0]) if G is None else G
    H, W = cshape if cshape else ((0, 0) if color is None else color.shape[1:3])
    Hd, Wd = dshape if dshape else ((0, 0) if depth is None else depth.shape[1:3])
    oh, ow = csize if csize else (0, 0)
    ohd, owd = dsize if dsize else (0, 0)
    n_c = 0 if color is None else color.shape[0] * 3 * oh * ow
    n_d = 0 if depth is None else depth.shape[0] * ohd * owd
    c_in = None if color is None else torch.from_numpy(np.ascontiguousarray(color)).to(cuda)
    d_in = None if depth is None else torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(cuda)
    c_out = torch.full((max(n_c, 0) + GUARD,), float("nan"), device=cuda)
    d_out = torch.full((max(n_d, 0) + GUARD,), float("nan"), device=cuda)
    ptr = lambda t, null: None if (t is None or null) else t.data_ptr()
    rc = L.pcrcg_prepare_frames(ptr(c_in, color_null), F, H, W, oh, ow, ptr(c_out if color is not None else None, color_null),
                                ptr(d_in, depth_null), G, Hd, Wd, ohd, owd, ptr(d_out if depth is not None else None, depth_null),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c_host, d_host = c_out.cpu().numpy(), d_out.cpu().numpy()
    assert np.isnan(c_host[max(n_c, 0):]).all() and np.isnan(d_host[max(n_d, 0):]).all(), "a store went past an output"
    got_c = None if color is None else c_host[:n_c].reshape(color.shape[0], 3, oh, ow)
    got_d = None if depth is None else d_host[:n_d].reshape(depth.shape[0], ohd, owd)
    return rc, got_c, got_d


def _frames(seed, F, shape, G, dshape):
    rng = np.random.RandomState(seed)
    color = rng.randint(0, 256, (F,) + tuple(shape) + (3,)).astype(np.uint8) if F else None
    depth = rng.randint(0, 65536, (G,) + tuple(dshape)).astype(np.uint16) if G else None
    return color, depth


def _check(got_c, got_d, color, csize, depth, dsize):
    if color is not None:
        assert not np.isnan(got_c).any()                                 # every pixel written
        for f in range(len(color)):
            assert got_c[f].tobytes() == IR.color_to_tensor(color[f], csize).tobytes(), f
    if depth is not None:
        assert not np.isnan(got_d).any()
        for g in range(len(depth)):
            assert got_d[g].tobytes() == IR.depth_to_tensor(depth[g], dsize).tobytes(), g


SIZES = [((1, 1), (5, 7)), ((3, 5), (9, 15)), ((3, 5), (7, 11)), ((480, 640), (1, 1)), ((7, 9), (7, 9)), ((4, 6), (2, 3)),
         ((6, 4), (4, 8)), ((8, 12), (2, 2))]


def test_the_cases_are_what_they_claim():
    exact = lambda n_in, n_out: ((np.arange(n_out) + 0.5) * n_in / n_out) % 1 == 0
    assert exact(4, 2).all() and exact(6, 3).all() and exact(8, 2).all() and exact(12, 2).all()   # an integer before the floor
    assert (IR.nearest_index(4, 2) == [1, 3]).all() and (IR.nearest_index(12, 2) == [3, 9]).all()
    assert (IR.nearest_index(1, 5) == 0).all() and (IR.nearest_index(480, 1) == [240]).all()
    assert (IR.nearest_index(3, 9) == np.repeat(np.arange(3), 3)).all()                            # up-scaling by 3
    assert (IR.nearest_index(7, 7) == np.arange(7)).all()
    assert (IR.nearest_index(4, 8) == np.repeat(np.arange(4), 2)).all() and (IR.nearest_index(6, 4) == [0, 2, 3, 5]).all()


@pytest.mark.parametrize("shape,size", SIZES)
def test_sizes(cuda, shape, size):
    """Two colour and two depth frames of `shape` to `size` in one call."""
    color, depth = _frames(shape[0] * 1000 + size[1], 2, shape, 2, shape)
    rc, c, d = _call(cuda, color, size, depth, size)
    assert rc == 0
    _check(c, d, color, size, depth, size)


def test_one_kind_only_with_null_pointers_for_the_other(cuda):
    color, depth = _frames(1, 3, (5, 4), 2, (6, 7))
    rc, c, d = _call(cuda, None, None, depth, (4, 9))                   # F = 0: the colour pointers are null, its sizes 0
    assert rc == 0 and c is None
    _check(None, d, None, None, depth, (4, 9))
    rc, c, d = _call(cuda, color, (7, 3), None, None)                   # G = 0
    assert rc == 0 and d is None
    _check(c, None, color, (7, 3), None, None)


def test_outputs_of_very_different_areas(cuda):
    """2000 colour pixels (eight workgroups a frame) beside 6 depth pixels, and 4200 depth pixels beside 2 colour pixels: the
    threads past the smaller output leave, every pixel of it is written and nothing behind it."""
    color, depth = _frames(2, 2, (3, 5), 3, (4, 6))
    rc, c, d = _call(cuda, color, (40, 50), depth, (2, 3))
    assert rc == 0
    _check(c, d, color, (40, 50), depth, (2, 3))
    color, depth = _frames(3, 3, (3, 5), 2, (7, 9))
    rc, c, d = _call(cuda, color, (1, 2), depth, (60, 70))
    assert rc == 0
    _check(c, d, color, (1, 2), depth, (60, 70))


def test_depth_at_the_int16_boundary(cuda):
    raw = np.array([[[0, 1, 32767], [32768, 65534, 65535]]], np.uint16)
    rc, _, d = _call(cuda, None, None, raw, (2, 3))
    assert rc == 0
    by_hand = np.array([0, 1, 32767, -32768, -2, -1], np.float32) / np.float32(1000)
    assert d.tobytes() == by_hand.reshape(1, 2, 3).tobytes()
    assert d.tobytes() == IR.depth_to_tensor(raw[0], (2, 3)).tobytes()
    assert d[0, 1, 2] == np.float32(-0.001) and d[0, 0, 2] == np.float32(32.767)


def test_colour_values_channel_by_channel(cuda):
    """Row c of the frame holds 0, 1, 127, 128, 254, 255 in channel c and 9 in the two others: plane c of the output holds
    them / 255 in row c and 9 / 255 elsewhere."""
    vals = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    frame = np.full((1, 3, 6, 3), 9, np.uint8)
    for ch in range(3):
        frame[0, ch, :, ch] = vals
    rc, c, _ = _call(cuda, frame, (3, 6), None, None)
    assert rc == 0
    want = np.full((3, 3, 6), np.float32(9) / np.float32(255), np.float32)
    for ch in range(3):
        want[ch, ch] = vals.astype(np.float32) / np.float32(255)
    assert c[0].tobytes() == want.tobytes()
    assert c[0].tobytes() == IR.color_to_tensor(frame[0], (3, 6)).tobytes()
    assert c[0, 0, 0, 5] == 1.0 and c[0, 2, 2, 0] == 0.0


def test_argument_errors_leave_the_outputs_alone(cuda):
    L = _lib.lib()
    color, depth = _frames(4, 1, (4, 5), 1, (3, 6))

    def refused(**kw):
        rc, c, d = _call(cuda, color, kw.pop("csize", (2, 2)), depth, kw.pop("dsize", (2, 2)), **kw)
        assert rc == EBADARG and b"bad argument" in L.pcrcg_last_error(), kw
        assert np.isnan(c).all() and np.isnan(d).all(), kw              # nothing was launched

    for bad in (0, 32769):
        refused(csize=(bad, 2))
        refused(csize=(2, bad))
        refused(dsize=(bad, 2))
        refused(dsize=(2, bad))
        refused(cshape=(bad, 5))
        refused(cshape=(4, bad))
        refused(dshape=(bad, 6))
        refused(dshape=(3, bad))
    refused(F=0, G=0)
    refused(F=65535, G=1)
    refused(F=1, G=65535)
    refused(F=-1)
    refused(color_null=True)
    refused(depth_null=True)
    rc, c, d = _call(cuda, color, (2, 2), depth, (2, 2))                 # and the same buffers are accepted as they are
    assert rc == 0
    _check(c, d, color, (2, 2), depth, (2, 2))
