"""GPU: colored ICP (csrc/colored.hip: pcrcg_color_gradients_batch, k_color_gradients; csrc/icp.hip: pcrcg_colored_icp_batch,
k_icp_evaluate<3>, k_icp_update<3>; csrc/colored_terms.h; registration.color_gradients_batch / colored_icp_batch) against the
numpy restatement tests/colored_icp_ref.py, whose rows, 3 x 3 solve and per-correspondence terms are the headers' own bit for
bit (tests/test_colored_terms_cpu.py).

Gradients: the lists' lengths exact, the nine sums within 1e-12 x the sums of the terms' absolute values, the gradient the
restated solve_ldlt3 of the DEVICE's own sums bit for bit; and, independent of the restatement, the tangential part of c on a
plane coloured I = c . x.

Steps: every traced iteration is recomputed from the device's own T_k, correspondences and records, with the three comparisons
and the bars of tests/test_gicp_gpu._check_steps:
  1. correspondences and counts exact, the 27 sums within 1e-12 x the sums of the terms' absolute values;
  2. T_k+1 against icp_plane_ref.step_from_sums(the device's own 27 sums, T_k) within 1e-12 max(1, max|T_k|, max|x|);
  3. T_k+1 against the np.longdouble solve of the RESTATED sums within 1e-13 cond(A) max|x| + FORM max(1, max|T_k|, max|x|).
tests/test_colored_icp_cpu.py::test_the_cases_are_what_they_claim checks on the CPU that no decision of these runs hangs on a
last bit.

Measured on an MI355X, the largest error over its bar of every step of every case of test_steps_follow_the_restatement:
comparison 1: 6.8e-3 (plane513); comparison 2: 1.1e-4; comparison 3: 3.1e-2 (size513, where the bar is FORM's 4e-15: cond(A) is
25).  The linear colour's gradients came within 4.3e-7 of their bar.  The textured plane ended 0.00088 / 0.0044 / 0.00088 from
the planted pose for 300 / 7 / 513 sources (from 0.063 / 0.051 / 0.059), as the restatement to the digits shown; point-to-plane
made no update on any of the three.
"""
import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

from . import colored_icp_ref as CR
from . import icp_plane_ref as PR
from . import icp_ref as IR
from .test_icp_plane_edges_gpu import FORM

pytestmark = pytest.mark.gpu

D, MI = CR.D, CR.MI


def _same_bits(a, b):
    """Equal bit for bit, a NaN standing for any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and a[~nan].tobytes() == b[~nan].tobytes()


# --- the gradients -------------------------------------------------------------------------------------------------------
def _wavy(seed, n, extent=0.25):
    """n points of a wavy sheet of `extent` with its exact unit normals and a colour per point -> pts fp32, normals, RGB.  Every
    fifth row from row 5 on repeats the row four before it: coincident points."""
    rng = np.random.RandomState(seed)
    u = rng.rand(n, 2) * extent
    pts = np.stack([u[:, 0], u[:, 1], 0.02 * np.sin(9 * u[:, 0]) * np.cos(7 * u[:, 1])], 1)
    gx, gy = 0.18 * np.cos(9 * u[:, 0]) * np.cos(7 * u[:, 1]), -0.14 * np.sin(9 * u[:, 0]) * np.sin(7 * u[:, 1])
    nrm = np.stack([-gx, -gy, np.ones(n)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    dup = np.arange(5, n, 5)
    pts[dup], nrm[dup] = pts[dup - 4], nrm[dup - 4]
    return pts.astype(np.float32), nrm, CR.texture(8.0 * pts + rng.rand(n, 1))


GRADIENT_SIZES = (0, 1, 3, 4, 5, 257)


@pytest.fixture(scope="module")
def clouds():
    return [_wavy(40 + i, n) for i, n in enumerate(GRADIENT_SIZES)]


def _check_gradients(pts, nrm, col, radius, max_nn, got):
    """One cloud's device gradients, counts and sums (host arrays) against the restatement -> the restatement's dict."""
    g, cnt, sums = got
    want = CR.gradients(pts, nrm, CR.intensity(col), radius, max_nn)
    assert np.array_equal(cnt, want["count"])
    finite = np.isfinite(want["sums"])
    assert (np.isfinite(sums) == finite).all()
    err = np.abs(sums - want["sums"])
    assert (err[finite] <= 1e-12 * want["mag"][finite]).all(), float((err[finite] / np.maximum(want["mag"][finite], 1e-300)).max())
    for k in range(len(pts)):
        x = CR.solve_ldlt3(sums[k, :6], sums[k, 6:]) if cnt[k] >= CR.MIN_LIST else None
        assert _same_bits(g[k], np.zeros(3) if x is None else x), k
        assert (x is not None) == bool(want["solved"][k]), k          # no solve hangs on the sums' last bits
    return want


@pytest.mark.parametrize("radius,max_nn", [(0.5, 30), (0.5, 64), (0.03, 30)])
def test_gradients_follow_the_restatement(cuda, clouds, radius, max_nn):
    """radius 0.5 covers every cloud: lists of 1, 3 (no gradient), exactly 4, 5, and 257 supports in the 27 cells cut to max_nn
    (the list of 128 is ranked and cut on the way); 0.03 leaves the large cloud lists of every length from 1 up."""
    pcds, nrms, cols = [c[0] for c in clouds], [c[1] for c in clouds], [c[2] for c in clouds]
    g, cnt, sums = REG.color_gradients_batch(pcds, cols, nrms, radius, max_nn, trace=True)
    wants = []
    for b, (pts, nrm, col) in enumerate(clouds):
        assert g[b].shape == (len(pts), 3) and g[b].dtype == torch.float64 and g[b].is_cuda
        wants.append(_check_gradients(pts, nrm, col, radius, max_nn, (g[b].cpu().numpy(), cnt[b].cpu().numpy(), sums[b].cpu().numpy())))
    big = wants[5]
    if radius == 0.5:
        assert [w["count"].tolist() for w in wants[:5]] == [[], [1], [3] * 3, [4] * 4, [5] * 5]
        assert not wants[2]["g"].any() and wants[3]["solved"].all() and wants[4]["solved"].all()
        assert (big["count"] == max_nn).all() and big["solved"].all()
    else:
        assert big["count"].min() < CR.MIN_LIST <= big["count"].max() < max_nn and big["solved"].sum() >= 200
    # coincident points: entry 0 is the lower index, for both rows of the pair
    for k in range(5, 257, 5):
        assert big["nbrs"][k][0] == k - 4 == big["nbrs"][k - 4][0]
    # the gradients are a view of the records: (n, g, I, 0)
    rec = g[5]._base
    assert rec.shape[1] == 8 and rec.data_ptr() % 64 == 0
    rows = rec[-257:].cpu().numpy()
    assert rows[:, :3].tobytes() == np.ascontiguousarray(clouds[5][1]).tobytes() and not rows[:, 7].any()
    assert rows[:, 6].tobytes() == CR.intensity(clouds[5][2]).tobytes()
    # a ragged batch equals its clouds alone, bit for bit; intensities in the place of RGB change nothing
    for b, (pts, nrm, col) in enumerate(clouds):
        alone = REG.color_gradients(pts, CR.intensity(col), torch.from_numpy(nrm).cuda(), radius, max_nn, trace=True)
        for x, y in zip(alone, (g[b], cnt[b], sums[b])):
            assert _same_bits(x.cpu().numpy(), y.cpu().numpy()), b
    two = REG.color_gradients_batch(pcds, cols, nrms, radius, max_nn, pairs_per_call=2)
    assert all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(two, g))


def test_a_nan_colour_stays_in_the_rows_whose_lists_hold_it(cuda, clouds):
    pts, nrm, col = clouds[5]
    clean = REG.color_gradients(pts, col, nrm, 0.03, 30).cpu().numpy()
    nbrs = CR.gradients(pts, nrm, CR.intensity(col), 0.03, 30)["nbrs"]
    for row in (0, 100, 256):
        dirty = col.copy()
        dirty[row, 1] = np.nan
        got = REG.color_gradients(pts, dirty, nrm, 0.03, 30).cpu().numpy()
        holds = np.array([len(nb) >= CR.MIN_LIST and (k == row or row in nb[1:]) for k, nb in enumerate(nbrs)])
        assert holds.sum() >= 2, row
        assert not np.isfinite(got[holds]).all(axis=1).any() and got[~holds].tobytes() == clean[~holds].tobytes(), row


def test_a_linear_colour_on_a_plane_gives_its_tangential_part(cuda):
    """I = c . x on the plane z = 0.25 (exact in fp32) with the normal (0, 0, 1): every neighbour lies in the tangent plane, so
    b_e = c . A_e up to the rounding of I, and every row with k >= 4 returns (c_x, c_y, 0) within
    1e-12 (cond(A^T A) max|c| + 1)."""
    rng = np.random.RandomState(2)
    n = 300
    pts = np.concatenate([rng.rand(n, 2), np.full((n, 1), 0.25)], 1).astype(np.float32)
    c = np.array([0.7, -0.4, 0.9])
    inten = pts.astype(np.float64) @ c
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))
    g, cnt, sums = (x.cpu().numpy() for x in REG.color_gradients(pts, inten, nrm, 0.12, 30, trace=True))
    rows = cnt >= CR.MIN_LIST
    assert rows.sum() >= 250
    worst = 0.0
    for k in np.flatnonzero(rows):
        cond = np.linalg.cond(_sym3(sums[k, :6]))
        err = np.abs(g[k] - np.array([0.7, -0.4, 0.0])).max()
        worst = max(worst, err / (1e-12 * (cond * 0.9 + 1.0)))
        assert err <= 1e-12 * (cond * 0.9 + 1.0), (k, err, cond)
    print(f"linear colour: largest error over its bar {worst:.2e}")


def _sym3(upper):
    A = np.zeros((3, 3))
    for e, (r, c) in enumerate(CR._UPPER3):
        A[r, c] = A[c, r] = upper[e]
    return A


# --- the steps -----------------------------------------------------------------------------------------------------------
def _host(trace, b):
    return {"T": trace["transforms"][b].cpu().numpy(), "counts": trace["counts"][b].cpu().numpy(),
            "sums": trace["sums"][b].cpu().numpy(), "corr": trace["corr"][b].cpu().numpy(),
            "sums27": trace["sums27"][b].cpu().numpy(), "rec": trace["tgt_records"][b].cpu().numpy(),
            "Is": trace["src_intensities"][b].cpu().numpy()}


def _check_steps(res, b, src, tgt, T0, lam=CR.LAMBDA, d=D, mi=MI):
    """Pair b of a traced result, one step at a time on the device's own records, with the three comparisons of the module's
    docstring -> (its host trace, the largest error over its bar of each comparison)."""
    tr = _host(res.trace, b)
    rec, Is = tr["rec"], tr["Is"]
    n = len(src)
    iters = int(res.iterations[b])
    assert 0 <= iters <= mi
    assert np.array_equal(tr["T"][0], np.asarray(T0, np.float64))
    can_update, worst = {}, [0.0, 0.0, 0.0]
    for k in range(iters + 1):
        Tk = tr["T"][k]
        corr, _, count, total = IR.evaluate(src, tgt, Tk, d)
        got = tr["corr"][k].astype(np.int64)
        assert (got == corr).all(), (k, np.flatnonzero(got != corr)[:5])
        assert tr["counts"][k] == count, k
        assert abs(tr["sums"][k] - total) <= 1e-12 * max(abs(total), 1e-300), k
        want, mag = CR.sums27(src, tgt, rec, Is, lam, Tk, got)
        finite = np.isfinite(want).all()
        if finite:
            err = np.abs(tr["sums27"][k] - want)
            assert (err <= 1e-12 * mag).all(), (k, err, mag)
            if count > 0:
                worst[0] = max(worst[0], float((err / np.maximum(mag, 1e-300)).max() / 1e-12))
        else:
            assert not np.isfinite(tr["sums27"][k]).all(), k
        same = PR.step_from_sums(tr["sums27"][k], Tk) if np.isfinite(tr["sums27"][k]).all() else None
        can_update[k] = count >= CR.MIN_COUNT and same is not None
        assert can_update[k] == (CR.update(src, tgt, rec, Is, lam, Tk, got)[0] is not None), k   # no decision hangs on the sums' last bits
        if k < iters:
            assert can_update[k], k
            A, rhs = PR.system(tr["sums27"][k])
            x = PR.solve_ldlt(A, rhs)
            size = max(1.0, np.abs(Tk).max(), np.abs(x).max())
            e2 = np.abs(tr["T"][k + 1] - same).max()
            Aw, bw = PR.system(want)
            cond = float(np.linalg.cond(Aw))
            xl = PR.solve_longdouble(Aw, bw)
            e3 = float(np.abs(tr["T"][k + 1] - PR.delta_longdouble(xl) @ Tk.astype(np.longdouble)).max())
            b2 = 1e-12 * size
            b3 = 1e-13 * cond * float(np.abs(xl).max()) + FORM * size
            print(f"step {k}: count {count}, cond {cond:.3e}, lowest pivot ratio {PR.pivot_ratios(A).min():.2e}, "
                  f"max|x| {np.abs(x).max():.2e}, same sums {e2:.2e} (bar {b2:.2e}), longdouble {e3:.2e} (bar {b3:.2e})")
            worst[1], worst[2] = max(worst[1], e2 / b2), max(worst[2], e3 / b3)
            assert e2 <= b2 and e3 <= b3, (k, e2, b2, e3, b3)
    assert IR.stop_iteration(tr["counts"], tr["sums"], n, lambda k: can_update[k], mi) == iters
    assert (tr["counts"][iters + 1:] == -1).all() and np.isnan(tr["T"][iters + 1:]).all()
    assert np.isnan(tr["sums27"][iters + 1:]).all() and np.isnan(tr["sums"][iters + 1:]).all()
    fit, rmse = IR.statistics(int(tr["counts"][iters]), float(tr["sums"][iters]), n)
    assert np.array_equal(res.matrices[b], tr["T"][iters])
    assert res.fitness[b] == fit and res.inlier_rmse[b] == rmse and res.counts[b] == tr["counts"][iters]
    return tr, tuple(float(w) for w in worst)


def _five(res, b):
    """The five outputs of pair b, as bytes and numbers that compare bit for bit."""
    return (res.matrices[b].tobytes(), np.float64(res.fitness[b]).tobytes(), np.float64(res.inlier_rmse[b]).tobytes(),
            int(res.counts[b]), int(res.iterations[b]))


def _run(cases, trace=False, **kw):
    """colored_icp_batch over cases (src, tgt, src RGB, tgt RGB, tgt normals, start, ...)."""
    kw.setdefault("max_iteration", MI)
    return REG.colored_icp_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases],
                                 np.stack([c[5] for c in cases]), D, tgt_normals=[c[4] for c in cases], trace=trace, **kw)


@pytest.mark.parametrize("name", CR.STEP_CASES)
def test_steps_follow_the_restatement(cuda, name):
    case = CR.case(name)
    src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = case
    reads = REG.D2H_READS
    res = _run([case], trace=True)
    assert REG.D2H_READS == reads + 1
    tr, worst = _check_steps(res, 0, src, tgt, start)
    print(f"{name}: updates {res.iterations[0]}, largest error / bar: sums {worst[0]:.2e}, same sums {worst[1]:.2e}, "
          f"longdouble {worst[2]:.2e}")
    # the records the steps read: the normals and intensities as given, the gradients the restatement's up to their sums' order
    assert tr["Is"].tobytes() == src_int.tobytes() and res.trace["normals"][0].cpu().numpy().tobytes() == nrm.tobytes()
    assert tr["rec"][:, [0, 1, 2, 6, 7]].tobytes() == rec[:, [0, 1, 2, 6, 7]].tobytes()
    assert ((tr["rec"][:, 3:6] != 0).any(1) == (rec[:, 3:6] != 0).any(1)).all()
    # (the nine sums agree within 1e-12 of their terms' sizes -- test_gradients_follow_the_restatement -- and cond(A^T A) <= 1e5 in
    # these cases -- tests/test_colored_icp_cpu.py -- so the solutions agree within 1e-7 of their size)
    assert np.abs(tr["rec"][:, 3:6] - rec[:, 3:6]).max() <= 1e-7 * max(1.0, np.abs(rec[:, 3:6]).max())
    run = CR.icp(src, tgt, rec, src_int, CR.LAMBDA, start, D, max_iteration=MI)
    assert res.iterations[0] == run[4] and res.counts[0] == run[3]
    if name in ("size1", "size5"):
        assert res.iterations[0] == 0 and res.matrices[0].tobytes() == start.tobytes()
    else:
        assert res.iterations[0] >= 2
    if name.startswith("plane"):
        assert res.fitness[0] == 1.0


def test_the_textured_plane_ends_where_the_restatement_ends(cuda):
    """Geometry is blind on the plane; colour is not.  The factor 2 is slack only: the steps are pinned to 1e-12 above."""
    for n in CR.PLANES:
        src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = CR.case(f"plane{n}")
        res = REG.colored_icp(src, tgt, cs, ct, None, D, tgt_normals=nrm)
        want = CR.icp(src, tgt, rec, src_int, CR.LAMBDA, start, D)
        a, b = PR.worst_displacement(src, res.matrix, T_gt), PR.worst_displacement(src, want[0], T_gt)
        began = PR.worst_displacement(src, start, T_gt)
        plane = REG.refine(src, tgt, None, D, estimation="point_to_plane", tgt_normals=nrm)
        print(f"plane{n}: from {began:.4f} to {a:.5f} in {res.iterations} updates (restatement {b:.5f} in {want[4]}); "
              f"point-to-plane: {plane.iterations} updates")
        assert a <= 2.0 * b and a < began / 4
        assert plane.iterations == 0 and plane.matrix.tobytes() == np.eye(4).tobytes()


def test_lambda_one_is_point_to_plane(cuda):
    cases = [CR.case("size1025"), CR.case("size513")]
    res = _run(cases, lambda_geometric=1.0, trace=True)
    want = REG.refine_batch([c[0] for c in cases], [c[1] for c in cases], np.stack([c[5] for c in cases]), D, max_iteration=MI,
                            estimation="point_to_plane", tgt_normals=[c[4] for c in cases], trace=True)
    for b in range(2):
        assert np.isfinite(res.trace["tgt_records"][b].cpu().numpy()).all()
        assert want.iterations[b] >= 2 and (want.trace["counts"][b].cpu().numpy()[:want.iterations[b] + 1] >= 6).all()
        assert np.array_equal(res.matrices[b], want.matrices[b]) and np.array_equal(res.fitness[b], want.fitness[b])
        assert np.array_equal(res.inlier_rmse[b], want.inlier_rmse[b])
        assert res.counts[b] == want.counts[b] and res.iterations[b] == want.iterations[b]
        assert np.array_equal(res.trace["sums27"][b].cpu().numpy(), want.trace["sums27"][b].cpu().numpy(), equal_nan=True)
    other = _run(cases)
    assert not np.array_equal(other.matrices, res.matrices)          # lambda reaches the kernel


# --- poisoned and empty input ----------------------------------------------------------------------------------------------
def test_a_nan_record_stops_its_pair_only_where_it_is_a_correspondence(cuda):
    src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = CR.case("size1025")
    clean = (src, tgt, cs, ct, nrm, start)
    want = _run([clean])
    assert want.iterations[0] >= 2
    corr0 = IR.evaluate(src, tgt, start, D)[0]
    assert (corr0 >= 0).all()
    nan_t = ct.copy()
    nan_t[corr0[17], 2] = np.nan
    nan_s = cs.copy()
    nan_s[1024, 0] = np.inf
    nan_n = nrm.copy()
    nan_n[corr0[3], 1] = np.nan
    for name, dirty in (("target colour", (src, tgt, cs, nan_t, nrm, start)), ("source colour", (src, tgt, nan_s, ct, nrm, start)),
                        ("normal", (src, tgt, cs, ct, nan_n, start))):
        res = _run([clean, dirty, clean], trace=True)
        tr, _ = _check_steps(res, 1, src, tgt, start)
        assert res.iterations[1] == 0 and res.matrices[1].tobytes() == start.tobytes(), name
        assert res.counts[1] == len(src) and res.fitness[1] == 1.0 and res.inlier_rmse[1] > 0, name
        assert not np.isfinite(tr["sums27"][0]).all(), name
        assert _five(res, 0) == _five(want, 0) == _five(res, 2), name         # the clean pairs beside it
    # a row that is nobody's correspondence, and in nobody's gradient list: far targets and a far source
    far_t = np.concatenate([tgt, np.array([[3.0, 3.0, 3.0]], np.float32)])
    far_s = np.concatenate([src, np.array([[-3.0, -3.0, -3.0]], np.float32)])
    grey, up = np.array([[0.5, 0.5, 0.5]]), np.array([[0.0, 0.0, 1.0]])
    base = _run([(far_s, far_t, np.concatenate([cs, grey]), np.concatenate([ct, grey]), np.concatenate([nrm, up]), start)], trace=True)
    assert _five(base, 0)[0] == _five(want, 0)[0] and base.iterations[0] == want.iterations[0]
    for k in range(base.iterations[0] + 1):
        corr = base.trace["corr"][0][k].cpu().numpy()
        assert corr[-1] == -1 and (corr != len(tgt)).all()
    for bad in (np.nan, np.inf):
        got = _run([(far_s, far_t, np.concatenate([cs, grey * bad]), np.concatenate([ct, grey * bad]),
                     np.concatenate([nrm, up * bad]), start)], trace=True)
        assert not np.isfinite(got.trace["tgt_records"][0][-1].cpu().numpy()).all()
        assert _five(got, 0) == _five(base, 0)
        a, b = _host(got.trace, 0), _host(base.trace, 0)
        for key in ("T", "counts", "sums", "sums27", "corr"):
            assert a[key].tobytes() == b[key].tobytes(), key


def test_empty_clouds_and_a_nan_start(cuda):
    src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = CR.case("size513")
    e3 = np.zeros((0, 3), np.float32)
    e3d = np.zeros((0, 3))
    cases = [(e3, tgt, e3d, ct, nrm, T_gt), (src, e3, cs, e3d, e3d, T_gt), (src, tgt, cs, ct, nrm, start), (src, tgt, cs, ct, nrm, start)]
    clean = _run(cases)
    for b in range(2):
        assert np.array_equal(clean.matrices[b], T_gt), b
        assert clean.fitness[b] == 0 and clean.inlier_rmse[b] == 0 and clean.counts[b] == 0 and clean.iterations[b] == 0, b
    assert clean.iterations[2] >= 2 and _five(clean, 2) == _five(clean, 3)
    bad = start.copy()
    bad[1, 2] = np.nan
    cases[2] = (src, tgt, cs, ct, nrm, bad)
    res = _run(cases)
    assert np.isnan(res.matrices[2]).all() and np.isnan(res.fitness[2]) and res.counts[2] == -1 and res.iterations[2] == -1
    for b in (0, 1, 3):
        assert _five(res, b) == _five(clean, b), b
    alone = _run([(e3, e3, e3d, e3d, e3d, np.eye(4))])
    assert alone.iterations[0] == 0 and alone.matrices[0].tobytes() == np.eye(4).tobytes()


def _c_entry(src, tgt, rec, src_int, start, n_max=None, mi=MI, lam=CR.LAMBDA):
    """One pair through pcrcg_colored_icp_batch on given records -> (transform [16], stats [4]) on the host."""
    L = _lib.lib()
    dev = torch.device("cuda")
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    n, m = len(src), len(tgt)
    offs = torch.tensor([0, n, 0, m, m], dtype=torch.int32, device=dev)
    gbytes = L.pcrcg_cellgrid_ws_bytes(m, 1)
    grid = torch.empty(gbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.pcrcg_cellgrid_build(t.data_ptr(), m, offs[4:].data_ptr(), 1, D, grid.data_ptr(), gbytes, st), "grid")
    wsb = L.pcrcg_colored_icp_batch_ws_bytes(1, n, m, mi)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.full((20,), -7.0, dtype=torch.float64, device=dev)
    recd, isd = torch.from_numpy(np.ascontiguousarray(rec)).to(dev), torch.from_numpy(np.ascontiguousarray(src_int)).to(dev)
    init = torch.from_numpy(np.ascontiguousarray(start, np.float64)).to(dev)
    _lib.check(L.pcrcg_colored_icp_batch(s.data_ptr(), offs.data_ptr(), n, n if n_max is None else n_max, offs[2:].data_ptr(), m,
                                         grid.data_ptr(), init.data_ptr(), 1, D, mi, 1e-6, 1e-6, lam, recd.data_ptr(), isd.data_ptr(),
                                         out.data_ptr(), out[16:].data_ptr(), None, ws.data_ptr(), wsb, st), "pcrcg_colored_icp_batch")
    h = out.cpu().numpy()
    return h[:16], h[16:]


def test_a_pair_longer_than_n_max_gets_nan_and_the_c_entry_is_the_python_entry(cuda):
    src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = CR.case("size1025")
    py = _run([(src, tgt, cs, ct, nrm, start)], trace=True)
    rec_d, is_d = py.trace["tgt_records"][0].cpu().numpy(), py.trace["src_intensities"][0].cpu().numpy()
    T, stats = _c_entry(src, tgt, rec_d, is_d, start, n_max=len(src) - 1)
    assert np.isnan(T).all() and np.isnan(stats).all()
    T, stats = _c_entry(src, tgt, rec_d, is_d, start)
    assert T.tobytes() == py.matrices[0].tobytes() and stats[3] == py.iterations[0] >= 2 and stats[2] == py.counts[0]


# --- batching ------------------------------------------------------------------------------------------------------------
RAGGED = ((0, 50), (1, 40), (64, 100), (700, 513), (1200, 1500))


@pytest.fixture(scope="module")
def ragged():
    """Five pairs of RAGGED's lengths: samples of the corner surface under the small pose with 1 mm noise, the texture on
    both, the surface's exact normals -> a list of (src, tgt, src RGB, tgt RGB, normals, start)."""
    out = []
    T = PR.small_pose()
    for i, (n, m) in enumerate(RAGGED):
        ps, pt = PR.corner(500 + i, n), PR.corner(600 + i, m)
        rng = np.random.RandomState(700 + i)
        tgt = pt @ T[:3, :3].T + T[:3, 3] + 0.001 * rng.randn(m, 3)
        out.append((ps.astype(np.float32).reshape(n, 3), tgt.astype(np.float32), CR.texture(ps.reshape(n, 3)), CR.texture(pt),
                    PR.corner_normals(pt) @ T[:3, :3].T, np.eye(4)))
    return out


def test_a_ragged_batch_equals_its_pairs_alone_bit_for_bit(cuda, ragged):
    reads = REG.D2H_READS
    batch = _run(ragged)
    assert REG.D2H_READS == reads + 1
    two = _run(ragged, pairs_per_call=2)
    assert REG.D2H_READS == reads + 2
    again = _run(ragged)
    rev = _run(ragged[::-1])
    for b, (n, m) in enumerate(RAGGED):
        alone = _run([ragged[b]])
        assert _five(batch, b) == _five(alone, 0) == _five(two, b) == _five(again, b) == _five(rev, 4 - b), (n, m)
        c = ragged[b]
        single = REG.colored_icp(c[0], c[1], c[2], c[3], c[5], D, tgt_normals=c[4], max_iteration=MI)
        assert (single.matrix.tobytes(), single.iterations) == (alone.matrices[0].tobytes(), alone.iterations[0])
    assert batch.iterations[0] == 0 and batch.counts[0] == 0 and batch.matrices[0].tobytes() == np.eye(4).tobytes()
    assert batch.iterations[1] == 0 and batch.counts[1] <= 1
    assert (batch.iterations[2:] >= 2).all()
    # numpy, device and mixed inputs; intensities in the place of RGB
    dev = torch.device("cuda", torch.cuda.current_device())
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    forms = {"device": lambda b, x: on(x), "mixed": lambda b, x: on(x) if b % 2 else x}
    for name, f in forms.items():
        got = REG.colored_icp_batch([f(b, c[0]) for b, c in enumerate(ragged)], [f(b + 1, c[1]) for b, c in enumerate(ragged)],
                                    [f(b, c[2]) for b, c in enumerate(ragged)], [f(b + 1, CR.intensity(c[3])) for b, c in enumerate(ragged)],
                                    on(np.stack([c[5] for c in ragged])) if name == "device" else None, D, max_iteration=MI,
                                    tgt_normals=[f(b, c[4]) for b, c in enumerate(ragged)])
        assert [_five(got, b) for b in range(5)] == [_five(batch, b) for b in range(5)], name


def test_a_fast_global_registration_result_as_the_start_adds_no_read(cuda):
    src, tgt, cs, ct, nrm, start, T_gt, rec, src_int = CR.case("size1025")
    order = np.random.RandomState(300 + PR.SIZES.index(1025)).permutation(1025)
    pairs = np.stack([order[::7], np.arange(0, 1025, 7)], 1)         # target j is source order[j]
    fgr = REG.fast_global_registration_batch([src, src], [tgt, tgt], maximum_correspondence_distance=0.05,
                                             correspondences=[pairs, pairs], seeds=[3, 4])
    assert isinstance(fgr, REG.FastGlobalRegistrationResult)
    run = lambda init: REG.colored_icp_batch([src, src], [tgt, tgt], [cs, cs], [ct, ct], init, D, tgt_normals=[nrm, nrm],
                                             max_iteration=MI)
    reads = REG.D2H_READS
    res = run(fgr)
    assert REG.D2H_READS == reads + 1
    by_array = run(fgr.matrices)
    for b in range(2):
        assert _five(res, b) == _five(by_array, b)
        assert PR.worst_displacement(src, res.matrices[b], T_gt) < 1e-6


def test_given_normals_and_a_normal_radius_agree_bit_for_bit(cuda, ragged):
    srcs, tgts = [c[0] for c in ragged[2:]], [c[1] for c in ragged[2:]]
    cs, ct = [c[2] for c in ragged[2:]], [c[3] for c in ragged[2:]]
    kw = dict(max_iteration=MI)
    reads = REG.D2H_READS
    inside = REG.colored_icp_batch(srcs, tgts, cs, ct, None, D, normal_radius=0.12, trace=True, **kw)
    assert REG.D2H_READS == reads + 1
    nt = REG.estimate_normals_batch(tgts, 0.12, 30)
    for b in range(3):
        assert torch.equal(inside.trace["normals"][b], nt[b])
    runs = [REG.colored_icp_batch(srcs, tgts, cs, ct, None, D, tgt_normals=nt, **kw),
            REG.colored_icp_batch(srcs, tgts, cs, ct, None, D, tgt_normals=[x.cpu().numpy() for x in nt], pairs_per_call=2, **kw),
            REG.colored_icp_batch(srcs, tgts, cs, ct, None, D, normal_radius=0.12, gradient_radius=2 * D, **kw)]
    for b in range(3):
        for r in runs:
            assert _five(r, b) == _five(inside, b), b
    assert (inside.iterations >= 1).all()
    # the gradient search reaches the kernel: another radius, other records
    other = REG.colored_icp_batch(srcs, tgts, cs, ct, None, D, tgt_normals=nt, gradient_radius=0.1, gradient_max_nn=12, trace=True, **kw)
    assert not torch.equal(other.trace["tgt_records"][2], inside.trace["tgt_records"][2])
    g = REG.color_gradients_batch(tgts, ct, nt, 0.1, 12)
    for b in range(3):
        assert torch.equal(other.trace["tgt_records"][b][:, 3:6], g[b])
