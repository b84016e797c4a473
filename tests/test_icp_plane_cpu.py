"""CPU: the numpy restatement of point-to-plane ICP (tests/icp_plane_ref.py) on pairs with a planted pose, and the host-side
argument checks of registration.refine_batch's estimator keywords."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import icp_plane_ref as PR
from . import icp_ref as IR
from . import normals_ref as NR

D = 0.15
R_NORMAL = 0.12


@pytest.fixture(scope="module")
def corner():
    src, tgt, T_gt = PR.corner_pair()
    return src, tgt, T_gt, NR.estimate(tgt, R_NORMAL, 30)["normals"]


def test_recovers_the_planted_pose(corner):
    src, tgt, T_gt, nrm = corner
    T, fit, rmse, count, k, hist = PR.icp(src, tgt, nrm, np.eye(4), D, max_iteration=30)
    err = np.abs(T - T_gt).max()
    print("updates", k, "fitness", fit, "rmse", rmse, "pose error", err, [float(np.abs(h[0] - T_gt).max()) for h in hist])
    assert fit == 1.0 and err < 1e-7
    assert k < 30                                     # the convergence test ended the loop, not the cap
    # fewer updates than point-to-point needs on the same pair
    T2, _, _, _, k2, _ = IR.icp(src, tgt, np.eye(4), D, max_iteration=30)
    print("point-to-point: updates", k2, "pose error", np.abs(T2 - T_gt).max())
    assert k < k2


def test_flipped_normals_change_no_bit(corner):
    src, tgt, T_gt, nrm = corner
    rng = np.random.RandomState(5)
    flipped = nrm * np.where(rng.rand(len(nrm)) < 0.5, -1.0, 1.0)[:, None]
    assert (flipped != nrm).any()
    a = PR.icp(src, tgt, nrm, np.eye(4), D, max_iteration=6)
    b = PR.icp(src, tgt, flipped, np.eye(4), D, max_iteration=6)
    assert a[4] == b[4] >= 1
    for (Ta, _, _), (Tb, _, _) in zip(a[5], b[5]):
        assert Ta.tobytes() == Tb.tobytes()


def test_the_system_is_well_conditioned_on_the_corner(corner):
    src, tgt, T_gt, nrm = corner
    corr = IR.evaluate(src, tgt, np.eye(4), D)[0]
    delta, cond = PR.update(src, tgt, nrm, np.eye(4), corr)
    assert delta is not None and cond <= 1e4
    A, b = PR.system(PR.sums27(src, tgt, nrm, np.eye(4), corr)[0])
    assert np.abs(PR.solve_ldlt(A, b) - np.linalg.solve(A, b)).max() < 1e-12


@pytest.mark.parametrize("tilted", [False, True])
def test_a_plane_is_degenerate_at_the_first_update(tilted):
    src, tgt, nrm, start = PR.plane_pair(tilted)
    corr = IR.evaluate(src, tgt, start, D)[0]
    assert (corr >= 0).sum() == len(src)
    assert PR.update(src, tgt, nrm, start, corr)[0] is None
    T, _, _, count, k, _ = PR.icp(src, tgt, nrm, start, D)
    assert k == 0 and count == len(src) and np.array_equal(T, start)


def test_fewer_than_six_correspondences_stop_the_pair(corner):
    src, tgt, T_gt, nrm = corner
    corr = IR.evaluate(src, tgt, T_gt, D)[0]
    few = np.full_like(corr, -1)
    few[:5] = corr[:5]
    assert PR.update(src, tgt, nrm, T_gt, few)[0] is None


def test_delta_is_open3d_s_vector_to_matrix():
    x = np.array([0.3, -0.2, 0.5, 1.0, 2.0, 3.0])
    D4 = PR.delta_of(x)
    assert np.allclose(D4[:3, :3] @ D4[:3, :3].T, np.eye(3), atol=1e-15) and np.array_equal(D4[:3, 3], x[3:])
    # small angles: R ~ I + [x]_x
    e = 1e-8
    S = PR.delta_of(np.array([e, 2 * e, 3 * e, 0, 0, 0]))[:3, :3] - np.eye(3)
    assert np.allclose(S, np.array([[0, -3 * e, 2 * e], [3 * e, 0, -e], [-2 * e, e, 0]]), atol=1e-15)


def test_estimator_keywords_are_checked_before_any_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")

    monkeypatch.setattr(REG, "_device", no_device)
    p, q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
    n7 = np.zeros((7, 3))
    with pytest.raises(ValueError, match="estimation"):
        REG.refine_batch([p], [q], None, 0.1, estimation="plane")
    with pytest.raises(ValueError, match="needs tgt_normals or a normal_radius"):
        REG.refine_batch([p], [q], None, 0.1, estimation="point_to_plane")
    with pytest.raises(ValueError, match="belong to"):
        REG.refine_batch([p], [q], None, 0.1, normal_radius=0.1)
    with pytest.raises(ValueError, match="belong to"):
        REG.refine_batch([p], [q], None, 0.1, tgt_normals=[n7])
    with pytest.raises(ValueError, match="not both"):
        REG.refine_batch([p], [q], None, 0.1, estimation="point_to_plane", tgt_normals=[n7], normal_radius=0.1)
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="normal radius"):
            REG.refine_batch([p], [q], None, 0.1, estimation="point_to_plane", normal_radius=bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_nn"):
            REG.refine_batch([p], [q], None, 0.1, estimation="point_to_plane", normal_radius=0.1, normal_max_nn=bad)
    with pytest.raises(ValueError, match="sets of target normals"):
        REG.refine_batch([p, p], [q, q], None, 0.1, estimation="point_to_plane", tgt_normals=[n7])
    with pytest.raises(ValueError, match="one row per target point"):
        REG.refine_batch([p], [q], None, 0.1, estimation="point_to_plane", tgt_normals=[np.zeros((6, 3))])
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        REG.refine_batch([p], [q], None, 0.1, estimation="point_to_plane", tgt_normals=[np.zeros((7, 2))])
    with pytest.raises(ValueError, match="estimation"):
        REG.refine(p, q, None, 0.1, estimation=1)


def test_the_tester_passes_the_estimator_through(monkeypatch):
    from pcrcg_amd import tester
    seen = []

    class Fake:
        matrices = np.zeros((1, 4, 4))

    def fake_refine_batch(src, tgt, init, d, **kw):
        seen.append((len(src[0]), len(tgt[0]), init, d, kw))
        return Fake()

    monkeypatch.setattr(REG, "refine_batch", fake_refine_batch)
    records = [{"pcd": np.zeros((12, 3), np.float32), "len_src": 5}]
    tester._refine_poses(records, "start", 0.05)
    tester._refine_poses(records, "start", 0.05, "point_to_plane", 0.1)
    assert seen[0] == (5, 7, "start", 0.05, {})                     # the call it always made
    assert seen[1] == (5, 7, "start", 0.05, {"estimation": "point_to_plane", "normal_radius": 0.1})


def test_without_a_device_the_entry_says_so(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p, q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.refine_batch([p], [q], None, 0.1, estimation="point_to_plane", normal_radius=0.1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.refine(p, q, None, 0.1, estimation="point_to_plane", tgt_normals=np.zeros((7, 3)))
