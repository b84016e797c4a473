"""CPU: the two numpy restatements of the voxel down-sampling agree bit for bit, the augmentation draws come in the
reference's order, prepare_pairs checks its arguments before it touches a device, and the library exports the entry."""
import ctypes
import random

import numpy as np
import pytest

from pcrcg_amd import _lib, kitti, kitti_config
from . import voxel_ref as VR


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(VR.single_cases()))
def test_the_two_restatements_agree_bit_for_bit(name):
    pts, voxel = VR.single_cases()[name]
    fast, literal = VR.voxel_down_sample(pts, voxel), VR.voxel_down_sample_literal(pts, voxel)
    for a, b in zip(fast, literal):
        assert _same_bits(a, b)
    rows, first, count = fast
    assert count.sum() == len(pts) and (np.diff(first) > 0).all() and rows.dtype == np.float64
    if len(pts):
        assert first[0] == 0


def test_restatements_on_the_shaped_inputs():
    """What each generator is for: one row per point, one row in all, one row per distinct point, rejected clouds."""
    assert len(VR.voxel_down_sample(VR.own_voxels(5000), 0.3)[0]) == 5000
    rows, first, count = VR.voxel_down_sample(VR.one_voxel(1500), 0.3)
    assert len(rows) == 1 and count[0] == 1500 and first[0] == 0
    rows, _, count = VR.voxel_down_sample(VR.duplicates(copies=4), 1e-3)
    assert (count % 4 == 0).all()
    assert VR.voxel_down_sample(VR.too_fine(), 0.3) is None and VR.voxel_down_sample_literal(VR.too_fine(), 0.3) is None
    bad = VR.cube(1, 10)
    bad[4, 1] = np.nan
    assert VR.voxel_down_sample(bad, 0.3) is None and VR.voxel_down_sample_literal(bad, 0.3) is None
    # a face point belongs to the voxel ABOVE the face: (p - vmin) / voxel is the exact integer
    pts = np.array([[-2.0, 0, 0], [-2.0 + 0.5 * 0.25, 0, 0], [np.nextafter(np.float32(-1.875), np.float32(-3)), 0, 0]], np.float32)
    _, first, count = VR.voxel_down_sample(pts, 0.25)
    assert first.tolist() == [0, 1] and count.tolist() == [2, 1]


def _reference_draws(n_src, n_tgt, cfg, seed):
    """ref:datasets/kitti.py:158-176 as written there, on numpy's and random's GLOBAL state."""
    np.random.seed(seed)
    random.seed(seed)
    out = [(np.random.rand(n_src, 3) - 0.5) * cfg.augment_noise, (np.random.rand(n_tgt, 3) - 0.5) * cfg.augment_noise]
    out.append(np.random.rand(3) * np.pi * 2)
    out.append(np.random.rand(1)[0] > 0.5)
    out.append(cfg.augment_scale_min + (cfg.augment_scale_max - cfg.augment_scale_min) * random.random())
    out.append(np.random.uniform(-cfg.augment_shift_range, cfg.augment_shift_range, 3))
    out.append(np.random.uniform(-cfg.augment_shift_range, cfg.augment_shift_range, 3))
    return out


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_augment_draws_in_the_reference_order(seed):
    cfg = kitti_config(augment_noise=0.01, augment_shift_range=2.0, augment_scale_max=1.2, augment_scale_min=0.8)
    d = kitti.augment_draws(37, 41, cfg, (np.random.RandomState(seed), random.Random(seed)))
    ns, nt, euler, flip, scale, ss, st = _reference_draws(37, 41, cfg, seed)
    assert _same_bits(d["noise_src"], ns) and _same_bits(d["noise_tgt"], nt) and _same_bits(d["euler"], euler)
    assert d["rotate_src"] == bool(flip) and d["scale"] == scale
    assert _same_bits(d["shift_src"], ss) and _same_bits(d["shift_tgt"], st)


def test_euler_zyx_matrix():
    """Rx(c) Ry(b) Rz(a): a proper rotation; one angle at a time it is the elementary rotation about z, y, x."""
    a = 0.3
    c, s = np.cos(a), np.sin(a)
    assert np.allclose(kitti.euler_zyx_matrix([a, 0, 0]), [[c, -s, 0], [s, c, 0], [0, 0, 1]], atol=1e-15)
    assert np.allclose(kitti.euler_zyx_matrix([0, a, 0]), [[c, 0, s], [0, 1, 0], [-s, 0, c]], atol=1e-15)
    assert np.allclose(kitti.euler_zyx_matrix([0, 0, a]), [[1, 0, 0], [0, c, -s], [0, s, c]], atol=1e-15)
    R = kitti.euler_zyx_matrix([1.1, 2.2, 3.3])
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) < 1e-14
    # extrinsic z, then y, then x: the z rotation is applied to a vector FIRST
    Rz, Ry, Rx = kitti.euler_zyx_matrix([1.1, 0, 0]), kitti.euler_zyx_matrix([0, 2.2, 0]), kitti.euler_zyx_matrix([0, 0, 3.3])
    assert np.allclose(R, Rx @ Ry @ Rz, atol=1e-15)


def test_prepare_pairs_checks_its_arguments():
    cfg = kitti_config()
    scan, M = np.zeros((5, 3), np.float32), np.eye(4)
    with pytest.raises(ValueError, match="no pairs"):
        kitti.prepare_pairs([], [], [], cfg)
    with pytest.raises(ValueError, match="list lengths differ"):
        kitti.prepare_pairs([scan], [scan, scan], [M], cfg)
    with pytest.raises(ValueError, match="list lengths differ"):
        kitti.prepare_pairs([scan], [scan], [M, M], cfg)
    with pytest.raises(ValueError, match="refined has 2 entries"):
        kitti.prepare_pairs([scan], [scan], [M], cfg, refined=[M, M])
    with pytest.raises(ValueError, match=r"scans1: cloud 0 must be an \[N, 3\] array"):
        kitti.prepare_pairs([scan], [np.zeros((5, 4), np.float32)], [M], cfg, refined=[M])
    with pytest.raises(ValueError, match=r"pair 0: the pose must be a \[4, 4\] transform"):
        kitti.prepare_pairs([scan], [scan], [np.eye(3)], cfg, refined=[M])
    with pytest.raises(ValueError, match=r"pair 0: the refined pose must be a \[4, 4\] transform"):
        kitti.prepare_pairs([scan], [scan], [M], cfg, refined=[np.eye(3)])


def test_voxel_down_sample_batch_checks_its_arguments():
    scan = np.zeros((5, 3), np.float32)
    with pytest.raises(ValueError, match="no clouds"):
        kitti.voxel_down_sample_batch([], 0.3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size must be positive and finite"):
            kitti.voxel_down_sample_batch([scan], bad)
    with pytest.raises(ValueError, match=r"cloud 1 must be an \[N, 3\] array"):
        kitti.voxel_down_sample_batch([scan, np.zeros(7, np.float32)], 0.3)


def test_library_exports_the_entry_and_rejects_bad_arguments():
    """No GPU: argument checks come before any launch.  (Without the symbols in the library the prototype lookup of
    _lib.lib() fails.)"""
    assert "pcrcg_voxel_down_sample_batch" in _lib.SIGNATURES and "pcrcg_voxel_down_sample_ws_bytes" in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.pcrcg_abi_version() == 4
    ws = lib.pcrcg_voxel_down_sample_ws_bytes
    assert ws(2, 240000) > 240000 * 40 and ws(1, 0) > 0 and ws(2, 240000) < 64 << 20
    assert ws(0, 10) == 0 and ws(65536, 10) == 0 and ws(1, -1) == 0 and ws(65535, 10) > 0
    p = ctypes.c_void_p(4096)      # fake non-null device pointers: nothing launches
    call = lambda pts=p, off=p, n=10, B=1, vs=0.3, out=p, ln=p, w=p, wsb=1 << 30: lib.pcrcg_voxel_down_sample_batch(
        pts, off, n, B, vs, out, ln, None, None, w, wsb, None)
    for kw in (dict(pts=None), dict(off=None), dict(out=None), dict(ln=None), dict(w=None), dict(B=0), dict(B=65536), dict(n=-1),
               dict(vs=0.0), dict(vs=-0.3), dict(vs=float("nan")), dict(vs=float("inf"))):
        assert call(**kw) == -1, kw
        assert b"bad argument" in lib.pcrcg_last_error()
    assert call(wsb=ws(1, 10) - 1) == -2 and b"workspace too small" in lib.pcrcg_last_error()
