"""CPU: the numpy restatement of the ICP refinement (tests/icp_ref.py) on its own, and what registration.refine_batch /
refine_ground_truth decide on the host before any device is touched."""
import numpy as np
import pytest

from pcrcg_amd import registration as REG

from . import icp_ref as IR


def test_restatement_recovers_a_known_pose():
    """300 seeded points, 5 degrees and 5 cm, no noise, d = 0.2 (larger than any point's displacement: 0.05 + 0.0873 x the
    half diagonal 0.87 = 0.126).  The loop must end on its own criterion, and its last update must have been fitted to the
    true pairs; then T is the least-squares fit of pairs that are exact but for fp32 rounding, so (triangle inequality)
    every source point lands within (its final residual) + (the rounding of the target it was paired with) of where the
    true pose puts it, and the final rmse -- the distance from a minimum of 0 that the criterion accepted -- is below
    relative_rmse."""
    rel = 1e-6
    src, tgt, T_gt = IR.cube_pair(3, 300, 300, angle_deg=5.0, shift=0.05)
    truth = IR.evaluate(src, tgt, T_gt, 1e-3)[0]
    assert (truth >= 0).all() and len(set(truth.tolist())) == 300
    T, fit, rmse, count, iters, hist = IR.icp(src, tgt, np.eye(4), 0.2, max_iteration=100, relative_fitness=rel,
                                               relative_rmse=rel)
    assert 1 <= iters < 100, "the loop must end on its criterion, not on the cap"
    assert IR.converged(hist[-1][1], hist[-1][2], hist[-2][1], hist[-2][2], rel, rel)
    assert (IR.evaluate(src, tgt, hist[-2][0], 0.2)[0] == truth).all()
    assert fit == 1.0 and count == 300
    assert rmse < rel
    s64 = src.astype(np.float64)
    gap = np.linalg.norm((s64 @ T[:3, :3].T + T[:3, 3]) - (s64 @ T_gt[:3, :3].T + T_gt[:3, 3]), axis=1)
    rounding = np.sqrt(3) * IR.EPS32 * (np.abs(tgt).max() + 6 * (np.abs(src).sum(1).max() + 1))
    assert np.sqrt((gap ** 2).mean()) <= rmse + rounding
    rot, trans = IR.RR.pose_error(T, T_gt)
    print("pose error", rot, trans, "rmse", rmse, "iterations", iters)


def test_tie_rule_lowest_index_wins():
    src, tgt, want = IR.lattice_ties(0)
    corr, d2, count, total = IR.evaluate(src, tgt, np.eye(4), 0.1)
    assert len(src) == 180 and count == 180
    assert (d2 == np.float32(0.0625 ** 2)).all()
    assert (corr == want).all()
    # the planted pairs really are ties, and the winner is not always the same side
    left = np.array([np.flatnonzero((tgt == s - np.float32([0.0625, 0, 0])).all(1))[0] for s in src])
    right = np.array([np.flatnonzero((tgt == s + np.float32([0.0625, 0, 0])).all(1))[0] for s in src])
    assert (np.minimum(left, right) == want).all()
    assert 30 < (left < right).sum() < 150
    assert not IR.margins(src, tgt, np.eye(4), 0.1)[1].any()          # and the float64 margin calls none of them decided


def test_margins_leave_out_at_most_one_percent_of_the_gpu_test_clouds():
    """The clouds of tests/test_icp_gpu.py (uniform in the unit cube, d = 0.1): the rows that fp32 rounding could decide
    either way stay within the 1 % cap, checked here on the restatement alone."""
    for seed, n, m in [(1, 1300, 1300), (2, 513, 700), (3, 511, 300), (4, 512, 512)]:
        src, tgt, _ = IR.cube_pair(seed, n, m)
        nearest, decided = IR.margins(src, tgt, np.eye(4), 0.1)
        assert (~decided).mean() <= 0.01, (seed, n, m, (~decided).mean())
        corr = IR.evaluate(src, tgt, np.eye(4), 0.1)[0]
        hit = corr >= 0
        assert (corr[decided & hit] == nearest[decided & hit]).all()
        assert hit.sum() >= 3


def test_stop_iteration_follows_the_loop():
    src, tgt, _ = IR.cube_pair(5, 200, 200)
    T, fit, rmse, count, iters, hist = IR.icp(src, tgt, np.eye(4), 0.1, max_iteration=30)
    counts, sums = [], []
    for Tk, _, _ in hist:
        _, _, c, s = IR.evaluate(src, tgt, Tk, 0.1)
        counts.append(c)
        sums.append(s)
    counts += [-1] * (31 - len(counts))
    sums += [np.nan] * (31 - len(sums))
    assert IR.stop_iteration(counts, sums, 200, lambda k: True, 30) == iters
    assert IR.stop_iteration([2] + [-1] * 30, [0.1] + [np.nan] * 30, 200, lambda k: False, 30) == 0


def test_refine_ground_truth_composition(monkeypatch):
    """ref:datasets/kitti.py:111-120: ICP sees xyz0 @ R^T + t and xyz1, starts at the identity with 0.2 / 200, and the result
    is M @ T."""
    rng = np.random.RandomState(0)
    xyz0, xyz1 = rng.rand(50, 3).astype(np.float32), rng.rand(60, 3).astype(np.float32)
    M = np.eye(4)
    M[:3, :3] = IR.RR.random_rotation(rng)
    M[:3, 3] = rng.rand(3)
    T = np.eye(4)
    T[:3, :3] = IR.RR.random_rotation(rng)
    T[:3, 3] = rng.rand(3) * 0.1
    seen = {}

    class Fake:
        matrix = T

    def fake_refine(src, tgt, init, d, **kw):
        seen.update(src=src, tgt=tgt, init=init, d=d, kw=kw)
        return Fake()

    monkeypatch.setattr(REG, "refine", fake_refine)
    out = REG.refine_ground_truth(xyz0, xyz1, M)
    assert out.dtype == np.float64 and out.shape == (4, 4)
    assert np.array_equal(out, M @ T)
    want = (xyz0 @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    assert np.array_equal(np.asarray(seen["src"]), want) and seen["tgt"] is xyz1
    assert seen["init"] is None and seen["d"] == 0.2 and seen["kw"] == {"max_iteration": 200}
    with pytest.raises(ValueError, match=r"\[4, 4\]"):
        REG.refine_ground_truth(xyz0, xyz1, np.eye(3))


def test_refine_batch_checks_its_arguments_before_any_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")

    monkeypatch.setattr(REG, "_device", no_device)
    p = np.zeros((5, 3), np.float32)
    with pytest.raises(ValueError, match="list lengths differ"):
        REG.refine_batch([p, p], [p], None, 0.1)
    with pytest.raises(ValueError, match="no pairs"):
        REG.refine_batch([], [], None, 0.1)
    for bad in (np.eye(4), np.zeros((2, 4, 4)), np.zeros((1, 3, 4))):
        with pytest.raises(ValueError, match="init must be"):
            REG.refine_batch([p], [p], bad, 0.1)
    for d in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_correspondence_distance must be positive"):
            REG.refine_batch([p], [p], None, d)
    for mi in (0, -3):
        with pytest.raises(ValueError, match="max_iteration"):
            REG.refine_batch([p], [p], None, 0.1, max_iteration=mi)
    with pytest.raises(ValueError, match="relative_fitness and relative_rmse"):
        REG.refine_batch([p], [p], None, 0.1, relative_rmse=-1e-6)
    with pytest.raises(ValueError, match=r"pair 1: the target must be an \[N, 3\] array"):
        REG.refine_batch([p, p], [p, np.zeros((5, 2), np.float32)], None, 0.1)
    with pytest.raises(ValueError, match=r"init must be a \[4, 4\]"):
        REG.refine(p, p, np.zeros((1, 4, 4)), 0.1)
    with pytest.raises(AssertionError, match="a device was asked for"):          # valid arguments get that far
        REG.refine_batch([p], [np.zeros((0, 3), np.float32)], np.eye(4)[None], 0.1)


def test_c_entry_rejects_bad_arguments_before_any_launch():
    import ctypes
    from pcrcg_amd import _lib
    L = _lib.lib()
    assert L.pcrcg_icp_batch_ws_bytes(1, 5000, 5000, 30) >= 152 + 132 * 11
    assert L.pcrcg_icp_batch_ws_bytes(0, 1, 1, 1) == 0 and L.pcrcg_icp_batch_ws_bytes(1, -1, 1, 1) == 0
    assert L.pcrcg_icp_batch_ws_bytes(1, 1, 1, 0) == 0 and L.pcrcg_icp_batch_ws_bytes(65536, 1, 1, 1) == 0
    f = ctypes.c_void_p(4096)            # fake non-null device pointers: nothing launches

    def call(src=f, n_total=10, n_max=10, B=1, d=0.1, mi=5, rf=1e-6, rr=1e-6, ws_bytes=1 << 20, out=f):
        return L.pcrcg_icp_batch(src, f, n_total, n_max, f, 10, f, None, B, d, mi, rf, rr, out, f, None, f, ws_bytes, None)

    for kw in (dict(src=None), dict(out=None), dict(B=0), dict(B=65536), dict(n_total=-1), dict(n_max=11), dict(d=0.0),
               dict(d=float("nan")), dict(mi=0), dict(mi=65537), dict(rf=-1.0), dict(rr=float("nan"))):
        assert call(**kw) == -1, kw
        assert b"bad argument" in L.pcrcg_last_error()
    assert call(ws_bytes=64) == -2 and b"workspace too small" in L.pcrcg_last_error()
