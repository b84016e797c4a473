"""CPU: the numpy restatement of Generalized ICP (tests/gicp_ref.py) on pairs with a planted pose, the conditions the GPU
tests rely on, and the argument checks of registration.generalized_icp_batch / covariances_from_normals and of the C entries
pcrcg_covariances_from_normals / pcrcg_gicp_batch -- none of which needs a device."""
import ctypes

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

from . import gicp_ref as GR
from . import icp_plane_ref as PR
from . import icp_ref as IR
from . import normals_ref as NR


def test_a_case_worked_by_hand():
    """Three sources at T = I with identity covariances on both sides: M = 2 I, W = I / 2, and with G = -[p]x every
    correspondence adds [[G^T G, G^T], [G, I]] / 2 to A and -[G^T d, d] / 2 to b, d = p - q.  G^T G = |p|^2 I - p p^T.
      p1 = (2, 0, 0), q1 = (2, 0, 1): d = (0, 0, -1); G^T G = diag(0, 4, 4); G^T d = p x d = (0, 2, 0)
      p2 = (0, 2, 0), q2 = (1, 2, 0): d = (-1, 0, 0); G^T G = diag(4, 0, 4); p x d = (0, 0, 2)
      p3 = (0, 0, 4), q3 = (0, 2, 4): d = (0, -2, 0); G^T G = diag(16, 16, 0); p x d = (8, 0, 0)
    Rotation block: diag(20, 20, 8) / 2 = diag(10, 10, 4).  Mixed block G^T / 2 = [p]x / 2 summed: [p1 + p2 + p3]x / 2 with
    the sum (2, 2, 4): [[0, -2, 1], [2, 0, -1], [-1, 1, 0]].  Translation block 3 I / 2.
    b = -(sum p x d, sum d) / 2 = -(8, 2, 2, -1, -2, -1) / 2 = (-4, -1, -1, 0.5, 1, 0.5).  All dyadic: exact."""
    src = np.array([[2, 0, 0], [0, 2, 0], [0, 0, 4]], np.float32)
    tgt = np.array([[2, 0, 1], [1, 2, 0], [0, 2, 4]], np.float32)
    iso = GR.covariances_from_normals(np.zeros((3, 3)), 1.0)
    assert np.array_equal(iso, np.tile([1.0, 0, 0, 1, 0, 1], (3, 1)))
    corr = IR.evaluate(src, tgt, np.eye(4), 2.5)[0]
    assert corr.tolist() == [0, 1, 2]
    s, mag = GR.sums27(src, tgt, iso, iso, np.eye(4), corr)
    A, b = PR.system(s)
    want = np.array([[10.0, 0, 0, 0, -2, 1],
                     [0, 10.0, 0, 2, 0, -1],
                     [0, 0, 4.0, -1, 1, 0],
                     [0, 2, -1, 1.5, 0, 0],
                     [-2, 0, 1, 0, 1.5, 0],
                     [1, -1, 0, 0, 0, 1.5]])
    assert np.array_equal(A, want) and np.array_equal(b, np.array([-4.0, -1, -1, 0.5, 1, 0.5]))
    x = PR.solve_ldlt(A, b)
    assert np.abs(A @ x - b).max() < 1e-14
    # two correspondences are too few, three are enough
    few = corr.copy()
    few[2] = -1
    assert GR.update(src, tgt, iso, iso, np.eye(4), few)[0] is None
    assert GR.update(src, tgt, iso, iso, np.eye(4), corr)[0] is not None


def test_isotropic_covariances_end_where_point_to_point_ends():
    src, tgt, cs, ct, T0, T_gt = GR.case("noisy_iso")
    got = GR.icp(src, tgt, cs, ct, T0, GR.D, max_iteration=30)
    want = IR.icp(src, tgt, T0, GR.D, max_iteration=30)
    a, b = PR.worst_displacement(src, got[0], T_gt), PR.worst_displacement(src, want[0], T_gt)
    print(f"epsilon = 1: {got[4]} updates, worst point {a:.4e} m; point-to-point: {want[4]} updates, {b:.4e} m")
    assert got[4] < 30 and want[4] < 30                 # the convergence test ended both loops (measured: 20 and 20)
    assert abs(a - b) <= 1e-4                           # measured: 4.649e-3 against 4.653e-3, 4e-6 apart


def test_the_offset_pair_converges():
    src, tgt, cs, ct, T0, T_gt = GR.case("offset")
    T, fit, rmse, count, k, hist, conds = GR.icp(src, tgt, cs, ct, T0, GR.D, max_iteration=30)
    worst = PR.worst_displacement(src, T, T_gt)
    print(f"offset_pair(0): {k} updates, cond(A) {conds}, worst point {worst:.3e} m")
    assert fit == 1.0 and 2 <= k < 30
    assert worst < 1e-6                                 # measured: 1.3e-9
    assert max(conds) <= 1e4                            # measured: 28.8


def test_generalized_beats_plane_beats_point_on_independent_samples():
    src, tgt, cs, ct, T0, T_gt = GR.case("noisy")
    gicp = GR.icp(src, tgt, cs, ct, T0, GR.D, max_iteration=30)
    plane = PR.icp(src, tgt, NR.estimate(tgt, GR.R_NORMAL, 30)["normals"], T0, GR.D, max_iteration=30)
    point = IR.icp(src, tgt, T0, GR.D, max_iteration=30)
    w = [PR.worst_displacement(src, r[0], T_gt) for r in (gicp, plane, point)]
    print("worst point: generalized", w[0], gicp[4], "point-to-plane", w[1], plane[4], "point-to-point", w[2], point[4])
    assert w[0] < w[1] < w[2] and w[0] < 1e-3           # measured: 0.83 mm, 1.39 mm, 4.65 mm


def test_flipped_normals_change_no_bit():
    rng = np.random.RandomState(5)
    nrm = NR.estimate(PR.corner_pair()[1], GR.R_NORMAL, 30)["normals"]
    sign = np.where(rng.rand(len(nrm)) < 0.5, -1.0, 1.0)[:, None]
    assert (sign < 0).any() and (sign > 0).any()
    for eps in (1.0, 1e-3, 1e-6):
        assert GR.covariances_from_normals(nrm, eps).tobytes() == GR.covariances_from_normals(nrm * sign, eps).tobytes()


# the largest |W - W_longdouble| over max|W_longdouble| measured on the M of every correspondence of every step of the two runs
# below; the bound is ten times that.  It is why the GPU's sums are compared with the same-order restatement and never with
# np.linalg.inv: at epsilon = 1e-6 the inverse itself is only good to 5e-11.
ADJUGATE_MEASURED = {1e-3: 7.3e-14, 1e-6: 5.5e-11}


@pytest.mark.parametrize("epsilon", sorted(ADJUGATE_MEASURED))
def test_the_adjugate_inverse_against_longdouble(epsilon):
    worst = 0.0
    for name in ("offset", "noisy"):
        src, tgt, _, _, T0, _ = GR.case(name)
        cs = GR.covariances_from_normals(NR.estimate(src, GR.R_NORMAL, 30)["normals"], epsilon)
        ct = GR.covariances_from_normals(NR.estimate(tgt, GR.R_NORMAL, 30)["normals"], epsilon)
        run = GR.icp(src, tgt, cs, ct, T0, GR.D, max_iteration=GR.MI)
        assert run[4] >= 2
        for Tk, _, _ in run[5]:
            corr = IR.evaluate(src, tgt, Tk, GR.D)[0]
            hit = corr >= 0
            m6 = GR.metric_matrix(np.broadcast_to(Tk[:3, :3], (int(hit.sum()), 3, 3)), cs[hit], ct[corr[hit]])
            exact = GR.inverse_longdouble(m6)
            err = np.abs(GR.adjugate_inverse(m6) - exact).max(1) / np.abs(exact).max(1)
            worst = max(worst, float(err.max()))
    print(f"epsilon = {epsilon}: |W - longdouble| / max|W| <= {worst:.3e}")
    assert worst <= 10.0 * ADJUGATE_MEASURED[epsilon]


@pytest.mark.parametrize("name", GR.STEP_CASES)
def test_the_cases_are_what_they_claim(name):
    """What tests/test_gicp_gpu.py relies on, checked on the restatement's own run of every pair it compares step by step: no
    row of any evaluation is decided by fp32 rounding (icp_ref.margins: the distance threshold and the two nearest targets),
    cond(A) <= 1e4 and every pivot ratio at least 1e-5 (seven decades over the rule) wherever an update is made, and the count
    rule is met from the side the name says.  So no decision of the loop hangs on a last bit."""
    src, tgt, cs, ct, T0, T_gt = GR.case(name)
    assert cs.shape == (len(src), 6) and ct.shape == (len(tgt), 6) and np.isfinite(cs).all() and np.isfinite(ct).all()
    run = GR.icp(src, tgt, cs, ct, T0, GR.D, max_iteration=GR.MI)
    k = run[4]
    assert k < GR.MI
    for step, (Tk, _, _) in enumerate(run[5]):
        corr, _, count, _ = IR.evaluate(src, tgt, Tk, GR.D)
        nearest, decided = IR.margins(src, tgt, Tk, GR.D)
        assert decided.all(), (name, step, np.flatnonzero(~decided)[:5])
        assert (nearest[corr >= 0] == corr[corr >= 0]).all()
        if count >= GR.MIN_COUNT:
            A, b = PR.system(GR.sums27(src, tgt, cs, ct, Tk, corr)[0])
            ratios = PR.pivot_ratios(A)
            cond = np.linalg.cond(A)
            print(name, "step", step, "count", count, "cond", cond, "lowest pivot ratio", ratios.min())
            assert len(ratios) == 6 and ratios.min() >= 1e-5 and cond <= 1e4, (name, step, cond, ratios)
    count0 = IR.evaluate(src, tgt, T0, GR.D)[2]
    if name in ("two", "size1"):
        assert count0 == {"two": 2, "size1": 1}[name] and k == 0 and np.array_equal(run[0], T0)
    else:
        assert k >= 2 and count0 >= GR.MIN_COUNT and run[3] == (3 if name == "three" else len(src))
    if name == "three":
        assert count0 == 3


def _no_device(*a, **k):
    raise AssertionError("a device was asked for before the arguments were checked")


def test_the_batch_entry_checks_its_arguments_before_any_device(monkeypatch):
    monkeypatch.setattr(REG, "_device", _no_device)
    p, q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
    n5, n7, c5, c7 = np.zeros((5, 3)), np.zeros((7, 3)), np.zeros((5, 3, 3)), np.zeros((7, 3, 3))
    G = REG.generalized_icp_batch
    both = dict(src_normals=[n5], tgt_normals=[n7])
    with pytest.raises(ValueError, match="list lengths differ"):
        G([p], [q, q], None, 0.1, **both)
    with pytest.raises(ValueError, match="no pairs"):
        G([], [], None, 0.1)
    for bad in (0.0, -1e-3, 1.5, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            G([p], [q], None, 0.1, epsilon=bad, **both)
    with pytest.raises(ValueError, match="the src side needs"):
        G([p], [q], None, 0.1, tgt_normals=[n7])
    with pytest.raises(ValueError, match="the tgt side needs"):
        G([p], [q], None, 0.1, src_covariances=[c5])
    with pytest.raises(ValueError, match="the src side needs"):
        G([p], [q], None, 0.1)
    with pytest.raises(ValueError, match="src_covariances or src_normals, not both"):
        G([p], [q], None, 0.1, src_covariances=[c5], src_normals=[n5], tgt_normals=[n7])
    with pytest.raises(ValueError, match="tgt_covariances or tgt_normals, not both"):
        G([p], [q], None, 0.1, src_normals=[n5], tgt_normals=[n7], tgt_covariances=[c7])
    with pytest.raises(ValueError, match="normal_radius belongs to a side without"):
        G([p], [q], None, 0.1, normal_radius=0.1, **both)
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="normal radius"):
            G([p], [q], None, 0.1, normal_radius=bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_nn"):
            G([p], [q], None, 0.1, src_normals=[n5], normal_radius=0.1, normal_max_nn=bad)
    with pytest.raises(ValueError, match="2 sets of src normals for 1 pairs"):
        G([p], [q], None, 0.1, src_normals=[n5, n5], tgt_normals=[n7])
    with pytest.raises(ValueError, match="tgt covariances must be"):
        G([p], [q], None, 0.1, src_normals=[n5], tgt_covariances=[np.zeros((7, 6))])
    with pytest.raises(ValueError, match="src normals must be"):
        G([p], [q], None, 0.1, src_normals=[n7], tgt_normals=[n7])
    with pytest.raises(ValueError, match="src covariances must be"):
        G([p], [q], None, 0.1, src_covariances=[c7], tgt_normals=[n7])
    with pytest.raises(ValueError, match=r"init must be \[1, 4, 4\]"):
        G([p], [q], np.eye(4), 0.1, **both)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            G([p], [q], None, bad, **both)
    for bad in (0, (1 << 16) + 1):
        with pytest.raises(ValueError, match="max_iteration"):
            G([p], [q], None, 0.1, max_iteration=bad, **both)
    with pytest.raises(ValueError, match="relative_fitness"):
        G([p], [q], None, 0.1, relative_rmse=-1.0, **both)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        G([np.zeros((5, 2), np.float32)], [q], None, 0.1, **both)
    # the single-pair entry lifts its arguments and meets the same checks
    with pytest.raises(ValueError, match=r"init must be a \[4, 4\]"):
        REG.generalized_icp(p, q, np.eye(3), 0.1, src_normals=n5, tgt_normals=n7)
    with pytest.raises(ValueError, match="tgt normals must be"):
        REG.generalized_icp(p, q, None, 0.1, src_normals=n5, tgt_normals=n5)
    with pytest.raises(ValueError, match="epsilon"):
        REG.generalized_icp(p, q, None, 0.1, epsilon=2.0, normal_radius=0.1)


def test_the_covariance_builder_checks_its_arguments_before_any_device(monkeypatch):
    monkeypatch.setattr(REG, "_device", _no_device)
    for bad in (0.0, -1.0, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            REG.covariances_from_normals(np.zeros((4, 3)), bad)
    for bad in (np.zeros((4, 2)), np.zeros(3), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError, match=r"\[N, 3\]"):
            REG.covariances_from_normals(bad)


def test_without_a_device_the_entries_say_so(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p, q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.generalized_icp_batch([p], [q], None, 0.1, normal_radius=0.1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.generalized_icp(p, q, None, 0.1, src_normals=np.zeros((5, 3)), tgt_covariances=np.zeros((7, 3, 3)))
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.covariances_from_normals(np.zeros((4, 3)))


def test_refine_batch_keeps_its_two_estimators():
    p, q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
    with pytest.raises(ValueError) as e:
        REG.refine_batch([p], [q], None, 0.1, estimation="generalized")
    assert str(e.value) == ("refine_batch: estimation must be one of ['point_to_plane', 'point_to_point'], got 'generalized'")


def test_the_c_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    cov = lib.pcrcg_covariances_from_normals
    for eps in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert cov(fake, 4, eps, fake, None) == -1 and b"epsilon" in lib.pcrcg_last_error()
    assert cov(fake, -1, 0.5, fake, None) == -1 and b"pcrcg_covariances_from_normals" in lib.pcrcg_last_error()
    assert cov(None, 4, 0.5, fake, None) == -1 and cov(fake, 4, 0.5, None, None) == -1
    assert cov(None, 0, 0.5, None, None) == 0 and cov(fake, 0, 1.0, fake, None) == 0        # n = 0: nothing to launch
    ws_bytes = lib.pcrcg_gicp_batch_ws_bytes
    assert ws_bytes(2, 1000, 900, 30) == lib.pcrcg_icp_batch_ex_ws_bytes(2, 1000, 900, 30) > 0
    for args in ((0, 10, 10, 5), (65536, 10, 10, 5), (1, -1, 10, 5), (1, 10, -1, 5), (1, 10, 10, 0), (1, 10, 10, (1 << 16) + 1)):
        assert ws_bytes(*args) == 0, args
    good = dict(src=fake, src_off=fake, n_total=10, n_max=10, tgt_off=fake, m_total=12, grid=fake, init=None, B=1, d=0.1, mi=5,
                rf=1e-6, rr=1e-6, src_cov=fake, tgt_cov=fake, out_t=fake, out_s=fake, trace=None, ws=fake, wsb=1 << 20, stream=None)

    def call(**kw):
        return lib.pcrcg_gicp_batch(*{**good, **kw}.values())

    for kw in (dict(src_cov=None), dict(tgt_cov=None), dict(src=None), dict(src_off=None), dict(tgt_off=None), dict(grid=None),
               dict(out_t=None), dict(out_s=None), dict(ws=None), dict(B=0), dict(B=65536), dict(n_total=-1), dict(m_total=-1),
               dict(n_max=11), dict(d=0.0), dict(d=float("nan")), dict(mi=0), dict(mi=(1 << 16) + 1), dict(rf=-1.0),
               dict(rr=float("nan"))):
        assert call(**kw) == -1, kw
        assert b"pcrcg_gicp_batch: bad argument" in lib.pcrcg_last_error(), (kw, lib.pcrcg_last_error())
    assert call(src_cov=None) == -1 and b"src_cov" in lib.pcrcg_last_error()
    assert call(tgt_cov=None) == -1 and b"tgt_cov" in lib.pcrcg_last_error()
    assert call(wsb=64) == -2 and b"workspace too small" in lib.pcrcg_last_error()             # PCRCG_EWORKSPACE
    # pcrcg_icp_batch_ex still takes 0 or 1 alone
    ex = (fake, fake, 10, 10, fake, 12, fake, None, 1, 0.1, 5, 1e-6, 1e-6)
    for estimation in (2, 3, -1):
        assert lib.pcrcg_icp_batch_ex(*ex, estimation, fake, fake, fake, None, fake, 1 << 20, None) == -1
        assert b"pcrcg_icp_batch_ex: bad argument: estimation == 0 || estimation == 1" in lib.pcrcg_last_error()
