"""CPU: the numpy restatement of the FPFH descriptor (tests/fpfh_ref.py) on cases checked by hand, its own fragile shares on
the clouds the GPU tests compare on, and the host-side argument checks of registration.compute_fpfh_feature_batch and of the
C entry."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import fpfh_ref as FR
from . import normals_ref as NR

FRAGILE_CAP = 0.005


def test_five_coincident_points():
    """Every pair has d = 0, so f = (0, 0, 0): the middle bin of each group; D = 0 everywhere, so the FPFH part is empty."""
    pts = np.tile(np.float32([0.5, -1.0, 2.0]), (5, 1))
    out = FR.fpfh(pts, FR.random_normals(5, 0), 0.1, 100)
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert (out["k"] == 5).all()
    assert np.array_equal(out["hist"], np.tile((want / 25).astype(np.int64), (5, 1)))
    assert np.array_equal(out["fpfh"], np.tile(want, (5, 1)))
    assert not out["fragile_any"].any()


def test_two_points_give_the_pair_worked_by_hand():
    """p0 = 0 with n = z, p1 = (0.5, 0, 0) with n = (0.6, 0, 0.8).  From p0: a1 = 0, a2 = 0.6, so the pair is swapped: n1 =
    (0.6, 0, 0.8), dp = (-0.5, 0, 0), f2 = -0.6; v = dp x n1 = (0, 0.4, 0) / 0.4; w = n1 x v = (-0.8, 0, 0.6); f1 = 0;
    f0 = atan2(0.6, 0.8).  From p1 nothing is swapped and the same n1, dp come out.  Bins: floor(11 (0.6435 + pi) / 2 pi) = 6,
    floor(5.5) = 5, floor(2.2) = 2.  k = 2: SPFH = 100 per counted bin, and the neighbour's SPFH normalised to 100 on top."""
    pts = np.float32([[0, 0, 0], [0.5, 0, 0]])
    nrm = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
    f, frag = FR.pair_features(pts[0].astype(np.float64), nrm[0], pts[1:].astype(np.float64), nrm[1:])
    assert np.allclose(f[0], [np.arctan2(0.6, 0.8), 0.0, -0.6], atol=1e-15) and not frag.any()
    out = FR.fpfh(pts, nrm, 1.0, 100)
    want = np.zeros(33)
    want[[6, 11 + 5, 22 + 2]] = 200.0
    assert np.array_equal(out["k"], [2, 2])
    assert np.allclose(out["fpfh"], np.tile(want, (2, 1)), atol=1e-12)
    assert np.array_equal(out["hist"][0], (want / 200).astype(np.int64))
    alone = FR.fpfh(pts, nrm, 0.25, 100)                           # out of each other's radius: k = 1, zero rows
    assert np.array_equal(alone["k"], [1, 1]) and not alone["fpfh"].any()


def test_a_non_finite_normal_counts_in_no_bin():
    pts, nrm, r = FR.dense_cube()
    nrm = nrm.copy()
    nrm[7] = np.nan
    out, base = FR.fpfh(pts, nrm, r, 100), FR.fpfh(pts, FR.dense_cube()[1], r, 100)
    assert np.array_equal(out["k"], base["k"])
    assert not out["hist"][7].any()
    lists7 = np.array([7 in nb[1:] for nb in out["nbrs"]])
    assert (out["hist"][lists7].sum(1) == 3 * (out["k"][lists7] - 2)).all()
    assert np.array_equal(out["hist"][~lists7 & (np.arange(len(pts)) != 7)], base["hist"][~lists7 & (np.arange(len(pts)) != 7)])
    assert np.isfinite(out["fpfh"]).all()


@pytest.mark.parametrize("name", sorted(FR.PARITY))
def test_group_sums_and_fragile_share_on_the_parity_clouds(name):
    pts, nrm, r, ref = FR.parity_case(name)
    live = ref["k"] >= 2
    assert live.mean() > 0.99 and ref["k"].max() <= 100
    assert np.abs(FR.group_sums(ref["fpfh"][live]) - 200.0).max() <= 1e-9
    assert not ref["fpfh"][~live].any()
    assert (ref["hist"].sum(1) == 3 * np.maximum(ref["k"] - 1, 0)).all()
    assert ref["fragile_any"].mean() <= FRAGILE_CAP


def test_fragile_share_on_the_other_clouds():
    pts, nrm, r = FR.dense_cube()
    for k in (1, 2, 16, 64, 65, 128):
        ref = FR.fpfh(pts, nrm, r, k)
        assert ref["fragile_any"].mean() <= FRAGILE_CAP
        assert ref["k"].max() == min(k, 115)                       # up to 115 points lie in the radius
        live = ref["k"] >= 2
        if live.any():
            assert np.abs(FR.group_sums(ref["fpfh"][live]) - 200.0).max() <= 1e-9
    lat = NR.tie_lattice(0)
    for k in (4, 10):
        assert FR.fpfh(lat, FR.random_normals(len(lat), 130), 1.5 * 0.125, k)["fragile_any"].mean() <= FRAGILE_CAP
    hp, hn = FR.height_field()
    assert FR.fpfh(hp, hn, 0.25, 128)["fragile_any"].mean() <= FRAGILE_CAP


def test_arguments_are_checked_before_any_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")

    monkeypatch.setattr(REG, "_device", no_device)
    p = np.zeros((5, 3), np.float32)
    n = np.zeros((5, 3))
    with pytest.raises(ValueError, match="no clouds"):
        REG.compute_fpfh_feature_batch([], 0.1, normals=[])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            REG.compute_fpfh_feature_batch([p], bad, normals=[n])
    for bad in (0, 129, -3):
        with pytest.raises(ValueError, match="max_nn"):
            REG.compute_fpfh_feature_batch([p], 0.1, bad, normals=[n])
    for bad in (np.zeros((5, 2), np.float32), np.zeros(5, np.float32), np.zeros((5, 3, 1), np.float32)):
        with pytest.raises(ValueError, match=r"\[N, 3\]"):
            REG.compute_fpfh_feature_batch([p, bad], 0.1, normals=[n, n])
    with pytest.raises(ValueError, match="sets of normals"):
        REG.compute_fpfh_feature_batch([p, p], 0.1, normals=[n])
    for bad in (np.zeros((4, 3)), np.zeros((5, 2)), np.zeros(5)):
        with pytest.raises(ValueError, match="normals"):
            REG.compute_fpfh_feature_batch([p], 0.1, normals=[bad])
    with pytest.raises(ValueError, match="normal_radius"):
        REG.compute_fpfh_feature_batch([p], 0.1)
    for bad in (0.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            REG.compute_fpfh_feature_batch([p], 0.1, normal_radius=bad)
    with pytest.raises(ValueError, match="max_nn"):
        REG.compute_fpfh_feature_batch([p], 0.1, normal_radius=0.1, normal_max_nn=65)
    with pytest.raises(ValueError, match="viewpoints"):
        REG.compute_fpfh_feature_batch([p], 0.1, normal_radius=0.1, viewpoints=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="not both"):
        REG.compute_fpfh_feature_batch([p], 0.1, normals=[n], normal_radius=0.1)
    with pytest.raises(ValueError, match="viewpoint"):
        REG.compute_fpfh_feature(p, 0.1, normal_radius=0.1, viewpoint=np.zeros(4))
    with pytest.raises(ValueError, match="max_nn"):
        REG.compute_fpfh_feature(p, 0.1, 129, normals=n)


def test_the_c_entry_rejects_bad_arguments_before_any_launch():
    """Fake non-null device pointers: every call below returns before anything is launched or dereferenced."""
    import ctypes
    from pcrcg_amd import _lib
    lib = _lib.lib()
    f = ctypes.c_void_p(4096)

    def fpfh(pts=f, off=f, n_total=100, n_max=100, grid=f, B=1, radius=0.1, max_nn=100, normals=f, out=f, ws=f, ws_bytes=1 << 20):
        return lib.pcrcg_fpfh_batch(pts, off, n_total, n_max, grid, B, radius, max_nn, normals, out, None, None, None, ws,
                                    ws_bytes, None)

    for kw in (dict(pts=None), dict(off=None), dict(grid=None), dict(normals=None), dict(out=None), dict(ws=None), dict(B=0),
               dict(B=65536), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(max_nn=0), dict(max_nn=129),
               dict(n_max=101), dict(n_total=-1, n_max=0)):
        assert fpfh(**kw) == -1, kw
        assert b"bad argument" in lib.pcrcg_last_error()
    need = lib.pcrcg_fpfh_ws_bytes(1, 100, 100)
    assert need >= 101 * (40 + 4 * 100) and need < 1 << 20
    assert lib.pcrcg_fpfh_ws_bytes(1, 100, 128) > need > lib.pcrcg_fpfh_ws_bytes(1, 100, 1) > 0
    for bad in ((0, 100, 100), (65536, 100, 100), (1, -1, 100), (1, 100, 0), (1, 100, 129)):
        assert lib.pcrcg_fpfh_ws_bytes(*bad) == 0, bad
    assert fpfh(ws_bytes=need - 1) == -2
    assert b"workspace" in lib.pcrcg_last_error()


def test_without_a_device_the_entry_says_so(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p = np.zeros((5, 3), np.float32)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.compute_fpfh_feature_batch([p], 0.1, normals=[np.zeros((5, 3))])
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.compute_fpfh_feature(p, 0.1, normal_radius=0.2)
