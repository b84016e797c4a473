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


def test_the_cases_are_what_they_claim():
    """The conditions tests/test_icp_plane_edges_gpu.py and tests/test_smallsolve_cpu.py rely on, checked on the restatement."""
    # the ladder: the rungs 0, 10, 100 m update at every step with every pivot ratio 10 x above the rule, 1000 m is refused
    # 10 x below it (300 m, 4 x above, is left out)
    for s in PR.LADDER:
        src, tgt, T_gt, nrm, run = PR.ladder_case(s)
        assert run[4] >= 2 and run[1] == 1.0 and len(run[5]) == run[4] + 1
        lowest = min(PR.pivot_ratios(A).min() for A, _ in PR.ladder_systems(s))
        cond = np.linalg.cond(PR.ladder_systems(s)[0][0])
        worst = PR.worst_displacement(src, run[0], T_gt)
        print(f"s = {s}: cond(A) at T_0 {cond:.2e}, lowest pivot ratio {lowest:.2e}, updates {run[4]}, worst point {worst:.2e}")
        assert lowest >= 1e-11 and run[4] < PR.LADDER_MI
        for (A, b), (Tk, _, _) in zip(PR.ladder_systems(s), run[5]):
            assert PR.solve_ldlt(A, b) is not None and len(PR.pivot_ratios(A)) == 6
    src, tgt, T_gt, nrm, run = PR.ladder_case(PR.FAR)
    A, b = PR.ladder_systems(PR.FAR)[0]
    ratios = PR.pivot_ratios(A)
    failing = ratios[ratios <= PR.PIVOT_RATIO]
    print(f"s = {PR.FAR}: cond(A) at T_0 {np.linalg.cond(A):.2e}, pivot ratios {ratios}")
    assert len(failing) >= 1 and failing[0] <= 1e-13 and (ratios[:4] > 1e-11).all()
    assert run[4] == 0 and run[1] == 1.0 and np.array_equal(run[0], np.eye(4)) and PR.solve_ldlt(A, b) is None
    assert PR.step_from_sums(np.concatenate([A[np.triu_indices(6)], b]), np.eye(4)) is None
    for s in PR.LADDER + (PR.FAR,):
        src, tgt, T_gt = PR.offset_pair(s)
        assert src.min() >= s - 0.1 and IR.evaluate(src, tgt, T_gt, 0.01)[2] == len(src)
    # the near-plane pair: the lowest pivot ratio is small, and three to five decades above the rule
    assert PR.near_plane_pair.__defaults__[2] == 2e-3
    for tilt, (low, high) in PR.NEAR_PLANE_TILTS.items():
        src, tgt, nrm, start = PR.near_plane_pair(tilt=tilt)
        out = PR.icp(src, tgt, nrm, start, D, max_iteration=10)
        assert out[4] >= 1 and out[1] == 1.0
        for Tk, _, _ in out[5]:
            A, _ = PR.system(PR.sums27(src, tgt, nrm, Tk, IR.evaluate(src, tgt, Tk, D)[0])[0])
            ratios = PR.pivot_ratios(A)
            assert len(ratios) == 6 and low <= ratios.min() <= high, (tilt, ratios)
        assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-15 and (src[:, 2] != 0).sum() == len(src) - 300
    # the sizes: one update or more from six points on, none below; every start is its own
    starts = set()
    for i, n in enumerate(PR.SIZES):
        src, tgt, nrm, start = PR.sized_pair(i, n)
        assert len(src) == len(tgt) == len(nrm) == n
        starts.add(start.tobytes())
        out = PR.icp(src, tgt, nrm, start, D, max_iteration=10)
        assert IR.evaluate(src, tgt, start, D)[2] == n
        if n >= 6:
            assert out[4] >= 1, n
        else:
            assert out[4] == 0 and np.array_equal(out[0], start), n
        off = start @ np.linalg.inv(PR.planted_pose())
        angle = np.degrees(np.arccos(np.clip((np.trace(off[:3, :3]) - 1) / 2, -1, 1)))
        assert 0.8 <= angle <= 1.6 and 0.008 <= np.linalg.norm(off[:3, 3]) <= 0.03, (n, angle, off[:3, 3])
    assert len(starts) == len(PR.SIZES)


def test_pivot_ratios_and_step_from_sums_follow_the_solver():
    rng = np.random.RandomState(11)
    M = rng.randn(6, 9)
    A, b = M @ M.T, rng.randn(6)
    ratios = PR.pivot_ratios(A)
    assert len(ratios) == 6 and ratios[0] == 1.0 and (ratios > 0).all() and (ratios <= 1).all()
    s27 = np.concatenate([A[np.triu_indices(6)], b])
    T = PR.planted_pose()
    assert np.array_equal(PR.step_from_sums(s27, T), PR.delta_of(PR.solve_ldlt(A, b)) @ T)
    x = PR.solve_longdouble(A, b)
    assert np.abs(x.astype(np.float64) - np.linalg.solve(A, b)).max() < 1e-12
    assert np.abs(PR.delta_longdouble(x).astype(np.float64) - PR.delta_of(x.astype(np.float64))).max() < 1e-15
    A[2, :] = A[:, 2] = 0.0                                  # rank 5: the last pivot is 0 or rounding noise
    assert PR.pivot_ratios(A)[-1] <= 1e-13 and PR.step_from_sums(np.concatenate([A[np.triu_indices(6)], b]), T) is None


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
