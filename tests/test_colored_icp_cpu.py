"""CPU: the numpy restatement of colored ICP (tests/colored_icp_ref.py) on a case worked by hand and on the textured plane where
geometry alone is blind, the conditions the GPU tests rely on, and the argument checks of registration.color_gradients_batch /
colored_icp_batch and of the C entries pcrcg_color_gradients_batch / pcrcg_colored_icp_batch -- none of which needs a device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

from . import colored_icp_ref as CR
from . import icp_plane_ref as PR
from . import icp_ref as IR


def test_a_case_worked_by_hand():
    """Targets on the lattice {0, 1, 2}^2 of the plane z = 0 with the normal (0, 0, 1) and I = 0.5 x + 0.25 y; radius 1.25, so
    the centre (1, 1, 0) has itself and its four axis neighbours.  Rows A_e = (+-1, 0, 0), (0, +-1, 0) with b = +-0.5, +-0.25;
    last row 4 n: A^T A = diag(2, 2, 16), A^T b = (1, 0.5, 0), g = (0.5, 0.25, 0).  All dyadic: exact.
    One source at (1.25, 1, 0.5) with Is = 1 against the centre q = (1, 1, 0), It = 0.75, and sg = 0.5, sp = 2 given as they are:
      rG = 0.5; J = [p x n | n] = (1, -1.25, 0, 0, 0, 1); JG = (0.5, -0.625, 0, 0, 0, 0.5); rg = 0.25;
      e = (p - rG n) - q = (0.25, 0, 0); I0 = 0.5 x 0.25 + 0.75 = 0.875; ri = 2 (1 - 0.875) = 0.25;
      gM = (-0.5, -0.25, 0); p x gM = (1 x 0 - 0.5 x -0.25, 0.5 x -0.5 - 1.25 x 0, 1.25 x -0.25 - 1 x -0.5) = (0.125, -0.25, 0.1875);
      JI = 2 (0.125, -0.25, 0.1875, -0.5, -0.25, 0) = (0.25, -0.5, 0.375, -1, -0.5, 0);
      b = -(JG rg + JI ri) = -(0.125 + 0.0625, -0.15625 - 0.125, 0.09375, -0.25, -0.125, 0.125)."""
    ij = np.stack(np.meshgrid(np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 2)
    tgt = np.concatenate([ij, np.zeros((9, 1))], 1).astype(np.float32)
    nrm = np.tile([0.0, 0.0, 1.0], (9, 1))
    inten = 0.5 * tgt[:, 0].astype(np.float64) + 0.25 * tgt[:, 1]
    out = CR.gradients(tgt, nrm, inten, 1.25, 30)
    centre = 4
    assert tgt[centre].tolist() == [1.0, 1.0, 0.0] and out["count"][centre] == 5 and out["count"][0] == 3
    assert np.array_equal(out["sums"][centre], [2.0, 0, 0, 2.0, 0, 16.0, 1.0, 0.5, 0.0])
    assert np.array_equal(out["g"][centre], [0.5, 0.25, 0.0])
    assert not out["g"][0].any() and not out["sums"][0].any()                   # a corner: a list of 3, no gradient
    assert out["count"][1] == 4 and np.array_equal(out["g"][1], [0.5, 0.25, 0.0])   # an edge point: exactly 4
    rec = CR.records(nrm, out["g"], inten)
    assert np.array_equal(rec[centre], [0, 0, 1, 0.5, 0.25, 0, 0.75, 0])
    t = CR.terms_of([[1.25, 1.0, 0.5]], [[1.0, 1.0, 0.0]], rec[centre], [1.0], 0.5, 2.0)[0]
    A, b = PR.system(t)
    JG, JI = np.array([0.5, -0.625, 0, 0, 0, 0.5]), np.array([0.25, -0.5, 0.375, -1.0, -0.5, 0])
    assert np.array_equal(A, np.outer(JG, JG) + np.outer(JI, JI))
    assert np.array_equal(b, -np.array([0.1875, -0.28125, 0.09375, -0.25, -0.125, 0.125]))
    assert CR.intensity(np.array([[0.25, 0.5, 0.75]]))[0] == 0.5 and CR.weights(0.75) == (np.sqrt(0.75), 0.5)


@pytest.mark.parametrize("n", CR.PLANES)
def test_colour_finds_the_in_plane_pose_that_geometry_cannot(n):
    """The textured plane: a flat, smoothly coloured plane, n sources against 400 independent targets, the in-plane pose planted
    about 0.06 away.  Point-to-plane refuses at T_0 (its system is singular); the joint objective ends below a quarter of the
    planted displacement.  Measured (start -> end): n = 300: 0.0632 -> 0.00088; 7: 0.0512 -> 0.0044; 513: 0.0585 -> 0.00088."""
    src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = CR.case(f"plane{n}")
    began = PR.worst_displacement(src, start, T_gt)
    run = CR.icp(src, tgt, rec, src_int, CR.LAMBDA, start, CR.D)
    ended = PR.worst_displacement(src, run[0], T_gt)
    plane = PR.icp(src, tgt, nrm, start, CR.D)
    print(f"plane{n}: {began:.4f} -> {ended:.5f} in {run[4]} updates; point-to-plane: {plane[4]} updates")
    assert 0.05 < began < 0.07 and run[4] >= 2 and ended < began / 4
    assert plane[4] == 0 and np.array_equal(plane[0], start)
    # the in-plane part of the step is colour's: with lambda_geometric = 1 the restatement refuses too
    assert CR.update(src, tgt, rec, src_int, 1.0, start, IR.evaluate(src, tgt, start, CR.D)[0])[0] is None


def test_lambda_one_is_point_to_plane():
    src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = CR.case("size513")
    corr = IR.evaluate(src, tgt, start, CR.D)[0]
    a, _ = CR.sums27(src, tgt, rec, src_int, 1.0, start, corr)
    b, _ = PR.sums27(src, tgt, nrm, start, corr)
    assert np.array_equal(a, b) and rec[:, 3:6].any()


@pytest.mark.parametrize("name", CR.STEP_CASES)
def test_the_cases_are_what_they_claim(name):
    """What tests/test_colored_icp_gpu.py relies on, checked on the restatement's own run of every pair it compares step by step.
    No decision hangs on a last bit:
      rows: none of any evaluation is decided by fp32 rounding (icp_ref.margins: the distance threshold, the two nearest targets);
      the count against the minimum of 3: met from the side the name says;
      the pivot ratio against 1e-12: wherever count >= 3, the lowest ratio is at least 1e-6 (six decades over the rule), or the
        system is singular outright (rank < 6, the ratio under 1e-14: fewer equations than unknowns) -- size5 alone;
      the convergence differences against 1e-6: no |fitness_k - fitness_k-1| or |rmse_k - rmse_k-1| within 1 % of the bound;
      the list length against 4: the neighbour lists are fp32 arithmetic the restatement repeats exactly; a target's gradient
        solve has its lowest pivot ratio at least 1e-5 (seven decades over the rule; so cond(A^T A) <= 1e5), or no solve at all."""
    src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = CR.case(name)
    assert rec.shape == (len(tgt), 8) and np.isfinite(rec).all() and np.isfinite(src_int).all()
    g = CR.gradients(tgt, nrm, CR.intensity(ct), CR.R_GRADIENT, CR.NN_GRADIENT)
    fitted = g["count"] >= CR.MIN_LIST
    assert (g["solved"] == fitted).all()
    for k in np.flatnonzero(fitted):
        assert CR.pivot_ratios3(g["sums"][k, :6]).min() >= 1e-5, (name, k)
    big = int(name[4:]) >= 511 if name.startswith("size") else True
    assert fitted.all() if big else not fitted.any()            # the small sized pairs: lists under 4, zero gradients throughout
    run = CR.icp(src, tgt, rec, src_int, CR.LAMBDA, start, CR.D, max_iteration=CR.MI)
    k_end = run[4]
    for step, (Tk, fit, rmse) in enumerate(run[5]):
        corr, _, count, _ = IR.evaluate(src, tgt, Tk, CR.D)
        nearest, decided = IR.margins(src, tgt, Tk, CR.D)
        assert decided.all(), (name, step, np.flatnonzero(~decided)[:5])
        assert (nearest[corr >= 0] == corr[corr >= 0]).all()
        if count >= CR.MIN_COUNT:
            A, b = PR.system(CR.sums27(src, tgt, rec, src_int, CR.LAMBDA, Tk, corr)[0])
            ratios = PR.pivot_ratios(A)
            print(name, "step", step, "count", count, "cond", np.linalg.cond(A), "lowest pivot ratio", ratios.min())
            if name == "size5":
                assert np.linalg.matrix_rank(A) < 6 and ratios.min() < 1e-14
            else:
                assert len(ratios) == 6 and ratios.min() >= 1e-6, (name, step, ratios)
        if step > 0:
            for diff in (abs(fit - run[5][step - 1][1]), abs(rmse - run[5][step - 1][2])):
                assert not 0.99e-6 <= diff <= 1.01e-6, (name, step, diff)
    count0 = IR.evaluate(src, tgt, start, CR.D)[2]
    if name == "size1":
        assert count0 == 1 and k_end == 0 and np.array_equal(run[0], start)
    elif name == "size5":
        assert count0 == 5 and k_end == 0 and np.array_equal(run[0], start)      # enough rows, too few equations: the pivot rule's
    else:
        assert k_end >= 2 and count0 >= CR.MIN_COUNT and run[3] == len(src)


def _no_device(*a, **k):
    raise AssertionError("a device was asked for before the arguments were checked")


def test_the_batch_entry_checks_its_arguments_before_any_device(monkeypatch):
    monkeypatch.setattr(REG, "_device", _no_device)
    p, q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
    c5, c7, n7 = np.zeros((5, 3)), np.zeros(7), np.zeros((7, 3))
    C = REG.colored_icp_batch
    ok = dict(tgt_normals=[n7])
    with pytest.raises(ValueError, match="list lengths differ"):
        C([p], [q, q], [c5], [c7], None, 0.1, **ok)
    with pytest.raises(ValueError, match="no pairs"):
        C([], [], [], [], None, 0.1)
    for bad in (-1e-3, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_geometric"):
            C([p], [q], [c5], [c7], None, 0.1, lambda_geometric=bad, **ok)
    with pytest.raises(ValueError, match="needs tgt_normals or a normal_radius"):
        C([p], [q], [c5], [c7], None, 0.1)
    with pytest.raises(ValueError, match="tgt_normals or normal_radius, not both"):
        C([p], [q], [c5], [c7], None, 0.1, normal_radius=0.1, **ok)
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="normal radius"):
            C([p], [q], [c5], [c7], None, 0.1, normal_radius=bad)
        with pytest.raises(ValueError, match="gradient radius"):
            C([p], [q], [c5], [c7], None, 0.1, gradient_radius=bad, **ok)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_nn"):
            C([p], [q], [c5], [c7], None, 0.1, normal_radius=0.1, normal_max_nn=bad)
        with pytest.raises(ValueError, match="gradient max_nn"):
            C([p], [q], [c5], [c7], None, 0.1, gradient_max_nn=bad, **ok)
    with pytest.raises(ValueError, match="2 sets of target normals for 1 pairs"):
        C([p], [q], [c5], [c7], None, 0.1, tgt_normals=[n7, n7])
    with pytest.raises(ValueError, match="target normals must have one row"):
        C([p], [q], [c5], [c7], None, 0.1, tgt_normals=[np.zeros((5, 3))])
    with pytest.raises(ValueError, match="2 sets of source colours for 1 clouds"):
        C([p], [q], [c5, c5], [c7], None, 0.1, **ok)
    with pytest.raises(ValueError, match="the source colours must have one row per point"):
        C([p], [q], [np.zeros((7, 3))], [c7], None, 0.1, **ok)
    with pytest.raises(ValueError, match="the target colours must have one row per point"):
        C([p], [q], [c5], [np.zeros(5)], None, 0.1, **ok)
    for bad in (np.zeros((7, 4)), np.zeros((7, 3, 1)), np.zeros(())):
        with pytest.raises(ValueError, match=r"the target colours must be \[N, 3\] RGB or \[N\] intensities"):
            C([p], [q], [c5], [bad], None, 0.1, **ok)
    with pytest.raises(ValueError, match=r"init must be \[1, 4, 4\]"):
        C([p], [q], [c5], [c7], np.eye(4), 0.1, **ok)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            C([p], [q], [c5], [c7], None, bad, **ok)
    for bad in (0, (1 << 16) + 1):
        with pytest.raises(ValueError, match="max_iteration"):
            C([p], [q], [c5], [c7], None, 0.1, max_iteration=bad, **ok)
    with pytest.raises(ValueError, match="relative_fitness"):
        C([p], [q], [c5], [c7], None, 0.1, relative_rmse=-1.0, **ok)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        C([np.zeros((5, 2), np.float32)], [q], [c5], [c7], None, 0.1, **ok)
    # the single-pair entry lifts its arguments and meets the same checks
    with pytest.raises(ValueError, match=r"init must be a \[4, 4\]"):
        REG.colored_icp(p, q, c5, c7, np.eye(3), 0.1, tgt_normals=n7)
    with pytest.raises(ValueError, match="target normals must have one row"):
        REG.colored_icp(p, q, c5, c7, None, 0.1, tgt_normals=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="lambda_geometric"):
        REG.colored_icp(p, q, c5, c7, None, 0.1, lambda_geometric=2.0, normal_radius=0.1)


def test_the_gradient_entry_checks_its_arguments_before_any_device(monkeypatch):
    monkeypatch.setattr(REG, "_device", _no_device)
    p, c, n = np.zeros((5, 3), np.float32), np.zeros((5, 3)), np.zeros((5, 3))
    G = REG.color_gradients_batch
    with pytest.raises(ValueError, match="no clouds"):
        G([], [], [], 0.1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gradient radius"):
            G([p], [c], [n], bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_nn"):
            G([p], [c], [n], 0.1, bad)
    with pytest.raises(ValueError, match="2 sets of cloud's colours for 1 clouds"):
        G([p], [c, c], [n], 0.1)
    with pytest.raises(ValueError, match="colours must have one row per point"):
        G([p], [np.zeros(4)], [n], 0.1)
    with pytest.raises(ValueError, match="0 sets of normals for 1 clouds"):
        G([p], [c], [], 0.1)
    with pytest.raises(ValueError, match="the normals must have one row per point"):
        G([p], [c], [np.zeros((4, 3))], 0.1)
    with pytest.raises(ValueError, match=r"the normals must be an \[N, 3\]"):
        REG.color_gradients(p, c, np.zeros(5), 0.1)
    with pytest.raises(ValueError, match=r"the cloud must be an \[N, 3\]"):
        REG.color_gradients(np.zeros((5, 2)), c, n, 0.1)


def test_without_a_device_the_entries_say_so(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p, q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.colored_icp_batch([p], [q], [np.zeros(5)], [np.zeros((7, 3))], None, 0.1, normal_radius=0.1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.colored_icp(p, q, np.zeros((5, 3)), np.zeros(7), None, 0.1, tgt_normals=np.zeros((7, 3)))
    with pytest.raises(RuntimeError, match="no HIP device"):
        REG.color_gradients(p, np.zeros(5), np.zeros((5, 3)), 0.1)


def test_the_older_entries_keep_their_signatures():
    want = {"refine_batch": "(src_pcds, tgt_pcds, init, max_correspondence_distance, *, max_iteration=30, relative_fitness=1e-06, "
                            "relative_rmse=1e-06, pairs_per_call=None, trace=False, estimation='point_to_point', tgt_normals=None, "
                            "normal_radius=None, normal_max_nn=30)",
            "generalized_icp_batch": "(src_pcds, tgt_pcds, init, max_correspondence_distance, *, epsilon=0.001, src_covariances=None, "
                                     "tgt_covariances=None, src_normals=None, tgt_normals=None, normal_radius=None, normal_max_nn=30, "
                                     "max_iteration=30, relative_fitness=1e-06, relative_rmse=1e-06, pairs_per_call=None, trace=False)",
            "colored_icp_batch": "(src_pcds, tgt_pcds, src_colors, tgt_colors, init, max_correspondence_distance, *, "
                                 "lambda_geometric=0.968, tgt_normals=None, normal_radius=None, normal_max_nn=30, gradient_radius=None, "
                                 "gradient_max_nn=30, max_iteration=30, relative_fitness=1e-06, relative_rmse=1e-06, pairs_per_call=None, "
                                 "trace=False)",
            "color_gradients_batch": "(pcds, colors, normals, radius, max_nn=30, *, pairs_per_call=None, trace=False)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(REG, name))) == sig, name
    p, q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
    with pytest.raises(ValueError) as e:
        REG.refine_batch([p], [q], None, 0.1, estimation="colored")
    assert str(e.value) == "refine_batch: estimation must be one of ['point_to_plane', 'point_to_point'], got 'colored'"


def test_the_c_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    # the gradients: pcrcg_estimate_normals_batch's rules
    assert lib.pcrcg_color_gradients_ws_bytes(2, 1000) == lib.pcrcg_estimate_normals_ws_bytes(2, 1000) > 0
    for args in ((0, 10), (65536, 10), (1, -1)):
        assert lib.pcrcg_color_gradients_ws_bytes(*args) == 0, args
    good = dict(pts=fake, off=fake, n_total=10, n_max=10, grid=fake, B=1, radius=0.1, max_nn=30, normals=fake, intensity=fake, rec=fake,
                count=None, sums=None, ws=fake, wsb=1 << 12, stream=None)

    def grad(**kw):
        return lib.pcrcg_color_gradients_batch(*{**good, **kw}.values())

    for kw in (dict(pts=None), dict(off=None), dict(grid=None), dict(normals=None), dict(intensity=None), dict(rec=None), dict(ws=None),
               dict(B=0), dict(B=65536), dict(n_total=-1), dict(n_max=-1), dict(n_max=11), dict(radius=0.0), dict(radius=-1.0),
               dict(radius=float("nan")), dict(radius=1e18), dict(max_nn=0), dict(max_nn=65)):
        assert grad(**kw) == -1, kw
        assert b"pcrcg_color_gradients_batch" in lib.pcrcg_last_error(), (kw, lib.pcrcg_last_error())
    assert grad(wsb=8) == -2                                                                     # PCRCG_EWORKSPACE
    assert grad(n_total=0, n_max=0, pts=None, normals=None, intensity=None, rec=None) == 0       # nothing to launch
    # the refinement: pcrcg_gicp_batch's rules under its own name, lambda_geometric, the records and the intensities
    ws_bytes = lib.pcrcg_colored_icp_batch_ws_bytes
    assert ws_bytes(2, 1000, 900, 30) == lib.pcrcg_icp_batch_ex_ws_bytes(2, 1000, 900, 30) > 0
    for args in ((0, 10, 10, 5), (65536, 10, 10, 5), (1, -1, 10, 5), (1, 10, -1, 5), (1, 10, 10, 0), (1, 10, 10, (1 << 16) + 1)):
        assert ws_bytes(*args) == 0, args
    good = dict(src=fake, src_off=fake, n_total=10, n_max=10, tgt_off=fake, m_total=12, grid=fake, init=None, B=1, d=0.1, mi=5,
                rf=1e-6, rr=1e-6, lam=0.968, tgt_rec=fake, src_int=fake, out_t=fake, out_s=fake, trace=None, ws=fake, wsb=1 << 20,
                stream=None)

    def call(**kw):
        return lib.pcrcg_colored_icp_batch(*{**good, **kw}.values())

    for kw in (dict(tgt_rec=None), dict(src_int=None), dict(lam=-1e-9), dict(lam=1.0000001), dict(lam=float("nan")),
               dict(lam=float("inf")), dict(src=None), dict(src_off=None), dict(tgt_off=None), dict(grid=None), dict(out_t=None),
               dict(out_s=None), dict(ws=None), dict(B=0), dict(B=65536), dict(n_total=-1), dict(m_total=-1), dict(n_max=11),
               dict(d=0.0), dict(d=float("nan")), dict(mi=0), dict(mi=(1 << 16) + 1), dict(rf=-1.0), dict(rr=float("nan"))):
        assert call(**kw) == -1, kw
        assert b"pcrcg_colored_icp_batch: bad argument" in lib.pcrcg_last_error(), (kw, lib.pcrcg_last_error())
    assert call(tgt_rec=None) == -1 and b"tgt_rec" in lib.pcrcg_last_error()
    assert call(src_int=None) == -1 and b"src_intensity" in lib.pcrcg_last_error()
    assert call(lam=2.0) == -1 and b"lambda_geometric" in lib.pcrcg_last_error()
    assert call(wsb=64) == -2 and b"workspace too small" in lib.pcrcg_last_error()             # PCRCG_EWORKSPACE
    # pcrcg_icp_batch_ex still takes 0 or 1 alone
    ex = (fake, fake, 10, 10, fake, 12, fake, None, 1, 0.1, 5, 1e-6, 1e-6)
    for estimation in (2, 3, 4, -1):
        assert lib.pcrcg_icp_batch_ex(*ex, estimation, fake, fake, fake, None, fake, 1 << 20, None) == -1
        assert b"pcrcg_icp_batch_ex: bad argument: estimation == 0 || estimation == 1" in lib.pcrcg_last_error()
