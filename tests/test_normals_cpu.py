"""CPU: the numpy restatement of the normal estimation (tests/normals_ref.py) against scipy's KD-tree and on shapes whose
normals are known, and the host-side argument checks of registration.estimate_normals_batch."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import normals_ref as NR


def test_neighbour_lists_equal_a_kd_tree_query():
    """The hybrid search: the max_nn nearest within the radius, nearest first.  Random float64-distinct inputs have no ties at
    the cut or at the radius, where fp32 and float64 distances could order two points differently."""
    spatial = pytest.importorskip("scipy.spatial")
    for pts, r, k in ((NR.cube(1, 600), 0.15, 30), (NR.noisy_sphere(2, 600), 0.25, 10), (NR.cube(3, 200), 0.2, 64)):
        tree = spatial.cKDTree(pts.astype(np.float64))
        dist, idx = tree.query(pts.astype(np.float64), k=k, distance_upper_bound=r)
        got = NR.neighbours(pts, r, k)
        for i in range(len(pts)):
            want = idx[i][np.isfinite(dist[i])]
            assert np.array_equal(got[i], want), i
            assert got[i][0] == i


def test_ties_are_cut_in_index_order():
    pts = NR.tie_lattice(0)
    h = 0.125
    full = NR.neighbours(pts, 1.5 * h, 64)
    sizes = {len(x) for x in full}
    assert max(sizes) == 19 and min(sizes) == 7                    # interior: 1 + 6 + 12; a corner: 1 + 3 + 3
    for k in (4, 10):
        cut = NR.neighbours(pts, 1.5 * h, k)
        for i, (a, b) in enumerate(zip(full, cut)):
            assert np.array_equal(a[:k], b)
        inner = [i for i, a in enumerate(full) if len(a) == 19]
        i = inner[0]
        ring = full[i][1:7] if k == 4 else full[i][7:19]
        assert (np.diff(ring) > 0).all()                           # equal d2: ascending index


def test_sphere_normals_are_radial():
    pts = NR.noisy_sphere(0)
    out = NR.estimate(pts, 0.25, 30)
    radial = pts.astype(np.float64) / np.linalg.norm(pts.astype(np.float64), axis=1, keepdims=True)
    assert 8 <= out["count"].min() and out["count"].max() == 30
    assert np.median(np.abs((out["normals"] * radial).sum(1))) > 0.999
    assert NR.well_separated(out["eig"]).all()
    # the viewpoint is the centre: every normal points inwards; seen from far outside along +x, the near cap points outwards
    assert ((out["normals"] * radial).sum(1) < 0).all()
    far = NR.estimate(pts, 0.25, 30, viewpoint=(10.0, 0.0, 0.0))
    cap = pts[:, 0] > 0.5
    assert ((far["normals"][cap] * radial[cap]).sum(1) > 0).all()
    same = np.abs((far["normals"] * out["normals"]).sum(1))
    assert np.allclose(same, 1.0, atol=1e-12)


def test_the_three_test_clouds_are_well_separated():
    for pts, r in ((NR.noisy_sphere(0), 0.25), (NR.cube(0), 0.15), (NR.lattice_sphere(0), 0.25)):
        out = NR.estimate(pts, r, 30)
        ok = NR.well_separated(out["eig"]) | out["fallback"]
        assert ok.mean() >= 0.99


def test_sign_rule():
    n = np.array([0.0, 0.6, -0.8])
    p = np.array([1.0, 2.0, 3.0])
    assert np.array_equal(NR.orient(n, p, np.zeros(3)), n)                      # n . (0 - p) = 1.2
    assert np.array_equal(NR.orient(-n, p, np.zeros(3)), n)
    on_plane = p + np.array([5.0, 0.0, 0.0])                                     # n . (v - p) = 0 exactly
    assert np.array_equal(NR.orient(n, p, on_plane), n)                          # first non-zero component (y) positive
    assert np.array_equal(NR.orient(-n, p, on_plane), n)
    assert NR.sign_ok(n, p, on_plane) and not NR.sign_ok(-n, p, on_plane)


def test_degenerate_rows_fall_back():
    two = np.array([[0, 0, 0], [0.01, 0, 0]], np.float32)
    out = NR.estimate(two, 0.1, 30)
    assert out["fallback"].all() and np.array_equal(out["normals"], np.tile([0.0, 0.0, 1.0], (2, 1)))
    same = np.tile(np.float32([0.5, -1.0, 2.0]), (5, 1))
    out = NR.estimate(same, 0.1, 30)
    assert (out["count"] == 5).all() and out["fallback"].all() and not out["cov"].any()
    line = np.stack([np.arange(9) * 0.01, np.zeros(9), np.zeros(9)], 1).astype(np.float32)
    out = NR.estimate(line, 0.1, 30)
    assert not out["fallback"].any() and np.abs(out["normals"][:, 0]).max() < 1e-9


def test_arguments_are_checked_before_any_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")

    monkeypatch.setattr(REG, "_device", no_device)
    p = np.zeros((5, 3), np.float32)
    with pytest.raises(ValueError, match="no clouds"):
        REG.estimate_normals_batch([], 0.1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            REG.estimate_normals_batch([p], bad)
    for bad in (0, 65, -3):
        with pytest.raises(ValueError, match="max_nn"):
            REG.estimate_normals_batch([p], 0.1, bad)
    for bad in (np.zeros(3), np.zeros((2, 3)), np.zeros((1, 4))):
        with pytest.raises(ValueError, match="viewpoints"):
            REG.estimate_normals_batch([p], 0.1, viewpoints=bad)
    for bad in (np.zeros((5, 2), np.float32), np.zeros(5, np.float32), np.zeros((5, 3, 1), np.float32)):
        with pytest.raises(ValueError, match=r"\[N, 3\]"):
            REG.estimate_normals_batch([p, bad], 0.1)
    with pytest.raises(ValueError, match="viewpoint"):
        REG.estimate_normals(p, 0.1, viewpoint=np.zeros(4))


def test_the_c_entries_reject_bad_arguments_before_any_launch():
    """Fake non-null device pointers: every call below returns before anything is launched or dereferenced."""
    import ctypes
    from pcrcg_amd import _lib
    lib = _lib.lib()
    f = ctypes.c_void_p(4096)

    def normals(pts=f, off=f, n_total=100, n_max=100, grid=f, B=1, radius=0.1, max_nn=30, out=f, ws=f, ws_bytes=1 << 20):
        return lib.pcrcg_estimate_normals_batch(pts, off, n_total, n_max, grid, B, radius, max_nn, None, out, None, None, ws,
                                                ws_bytes, None)

    for kw in (dict(pts=None), dict(off=None), dict(grid=None), dict(out=None), dict(ws=None), dict(B=0), dict(B=65536),
               dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(max_nn=0), dict(max_nn=65),
               dict(n_max=101), dict(n_total=-1, n_max=0)):
        assert normals(**kw) == -1, kw
        assert b"bad argument" in lib.pcrcg_last_error()
    assert lib.pcrcg_estimate_normals_ws_bytes(1, 100) > 0
    assert lib.pcrcg_estimate_normals_ws_bytes(0, 100) == 0 and lib.pcrcg_estimate_normals_ws_bytes(1, -1) == 0
    assert normals(ws_bytes=lib.pcrcg_estimate_normals_ws_bytes(1, 100) - 1) == -2

    def icp(estimation=1, normals=f, ws_bytes=1 << 20, B=1, n_max=100):
        return lib.pcrcg_icp_batch_ex(f, f, 100, n_max, f, 100, f, None, B, 0.1, 5, 1e-6, 1e-6, estimation, normals, f, f, None, f,
                                      ws_bytes, None)

    for kw in (dict(estimation=2), dict(estimation=-1), dict(normals=None), dict(B=0), dict(n_max=101)):
        assert icp(**kw) == -1, kw
        assert b"bad argument" in lib.pcrcg_last_error()
    need0, need1 = lib.pcrcg_icp_batch_ws_bytes(1, 100, 100, 5), lib.pcrcg_icp_batch_ex_ws_bytes(1, 100, 100, 5)
    assert need1 > need0 > 0
    assert icp(ws_bytes=need1 - 1) == -2 and icp(estimation=0, normals=None, ws_bytes=need0 - 1) == -2
    assert lib.pcrcg_icp_batch_ex_ws_bytes(0, 100, 100, 5) == 0 and lib.pcrcg_icp_batch_ex_ws_bytes(1, 100, 100, 0) == 0


def test_without_a_device_the_entry_says_so(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p = np.zeros((5, 3), np.float32)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.estimate_normals_batch([p], 0.1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.estimate_normals(p, 0.1, viewpoint=(0.0, 0.0, 1.0))
