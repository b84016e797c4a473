"""GPU: Generalized ICP (csrc/icp.hip: pcrcg_gicp_batch, k_icp_evaluate<2>, k_icp_update<2>, k_cov_from_normals;
csrc/gicp_terms.h; registration.generalized_icp_batch / covariances_from_normals) against the numpy restatement
tests/gicp_ref.py, whose per-correspondence terms are the header's own bit for bit (tests/test_gicp_terms_cpu.py).

Every traced iteration is recomputed from the device's own T_k and correspondences, with the three comparisons and the bars of
tests/test_icp_plane_edges_gpu._check_steps_split:
  1. correspondences and counts exact, the 27 sums within 1e-12 x the sums of the terms' absolute values;
  2. T_k+1 against icp_plane_ref.step_from_sums(the device's own 27 sums, T_k) within 1e-12 max(1, max|T_k|, max|x|);
  3. T_k+1 against the np.longdouble solve of the RESTATED sums within 1e-13 cond(A) max|x| + FORM max(1, max|T_k|, max|x|).
tests/test_gicp_cpu.py::test_the_cases_are_what_they_claim checks on the CPU that no decision of these runs hangs on a last bit.

Measured on an MI355X, the largest error over its bar of every step of every case of test_steps_follow_the_restatement:
comparison 1: 1.2e-2 (size1025); comparison 2: 1.1e-4; comparison 3: 5.4e-2 (size1025, where the bar is FORM's 4e-15: the
conditioning's share is below it, cond(A) being 24).  offset_pair(0) ended 1.3e-9 m from the planted pose after 3 updates, as the
restatement; with epsilon = 1 the noisy pair ended at 4.6489e-3 m after 20 updates, point-to-point at 4.6530e-3 m after 20.
"""
import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

from . import gicp_ref as GR
from . import icp_plane_ref as PR
from . import icp_ref as IR
from .test_icp_plane_edges_gpu import FORM

pytestmark = pytest.mark.gpu

D, MI, R_NORMAL = GR.D, GR.MI, GR.R_NORMAL


def _host(trace, b):
    return {"T": trace["transforms"][b].cpu().numpy(), "counts": trace["counts"][b].cpu().numpy(),
            "sums": trace["sums"][b].cpu().numpy(), "corr": trace["corr"][b].cpu().numpy(),
            "sums27": trace["sums27"][b].cpu().numpy()}


def _check_steps(res, b, src, tgt, cs, ct, T0, d=D, mi=MI):
    """Pair b of a traced result, one step at a time, with the three comparisons of the module's docstring -> (its host trace,
    the largest error over its bar of each comparison)."""
    tr = _host(res.trace, b)
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
        want, mag = GR.sums27(src, tgt, cs, ct, Tk, got)
        finite = np.isfinite(want).all()
        if finite:
            err = np.abs(tr["sums27"][k] - want)
            assert (err <= 1e-12 * mag).all(), (k, err, mag)
            if count > 0:
                worst[0] = max(worst[0], float((err / np.maximum(mag, 1e-300)).max() / 1e-12))
        else:
            assert not np.isfinite(tr["sums27"][k]).all(), k
        same = PR.step_from_sums(tr["sums27"][k], Tk) if np.isfinite(tr["sums27"][k]).all() else None
        can_update[k] = count >= GR.MIN_COUNT and same is not None
        assert can_update[k] == (GR.update(src, tgt, cs, ct, Tk, got)[0] is not None), k     # no decision hangs on the sums' last bits
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
    """generalized_icp_batch over gicp_ref cases (src, tgt, C_s [n,6], C_t [m,6], start, ...), covariances in open3d's layout."""
    kw.setdefault("max_iteration", MI)
    return REG.generalized_icp_batch([c[0] for c in cases], [c[1] for c in cases], np.stack([c[4] for c in cases]), D,
                                     src_covariances=[GR.unpack(c[2]) for c in cases],
                                     tgt_covariances=[GR.unpack(c[3]) for c in cases], trace=trace, **kw)


# --- the covariance builder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_the_builder_equals_the_restatement_bit_for_bit(cuda, n):
    rng = np.random.RandomState(n)
    nrm = rng.randn(n, 3)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    for eps in (1e-3, 1.0, 1e-6):
        got = REG.covariances_from_normals(nrm, eps)
        assert got.shape == (n, 6) and got.dtype == torch.float64 and got.is_cuda
        assert got.cpu().numpy().tobytes() == GR.covariances_from_normals(nrm, eps).tobytes()
        assert torch.equal(got, REG.covariances_from_normals(torch.from_numpy(-nrm).cuda(), eps))
    assert torch.equal(REG.covariances_from_normals(nrm), REG.covariances_from_normals(nrm, 1e-3))


def test_a_nan_normal_stays_in_its_row(cuda):
    rng = np.random.RandomState(3)
    nrm = rng.randn(257, 3)
    clean = REG.covariances_from_normals(nrm).cpu().numpy()
    for row in (0, 100, 255, 256):
        dirty = nrm.copy()
        dirty[row, 1] = np.nan
        got = REG.covariances_from_normals(dirty).cpu().numpy()
        keep = np.arange(257) != row
        assert got[keep].tobytes() == clean[keep].tobytes() and np.isnan(got[row]).any()
        want = GR.covariances_from_normals(dirty, 1e-3)
        assert (np.isnan(got[row]) == np.isnan(want[row])).all()


# --- the steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GR.STEP_CASES)
def test_steps_follow_the_restatement(cuda, name):
    case = GR.case(name)
    src, tgt, cs, ct, start, T_gt = case
    reads = REG.D2H_READS
    res = _run([case], trace=True)
    assert REG.D2H_READS == reads + 1
    assert res.trace["src_covariances"][0].cpu().numpy().tobytes() == cs.tobytes()
    assert res.trace["tgt_covariances"][0].cpu().numpy().tobytes() == ct.tobytes()
    tr, worst = _check_steps(res, 0, src, tgt, cs, ct, start)
    print(f"{name}: updates {res.iterations[0]}, largest error / bar: sums {worst[0]:.2e}, same sums {worst[1]:.2e}, "
          f"longdouble {worst[2]:.2e}")
    count0 = int(tr["counts"][0])
    if name in ("two", "size1"):
        assert count0 == {"two": 2, "size1": 1}[name] and res.iterations[0] == 0 and res.matrices[0].tobytes() == start.tobytes()
    else:
        assert res.iterations[0] >= 2
        if name == "three":
            assert count0 == 3 and res.counts[0] == 3
    if name == "offset":
        worst_point = PR.worst_displacement(src, res.matrices[0], T_gt)
        print("offset: worst point", worst_point)
        assert worst_point < 1e-6 and res.fitness[0] == 1.0


def test_isotropic_covariances_end_where_point_to_point_ends(cuda):
    case = GR.case("noisy_iso")
    src, tgt, cs, ct, start, T_gt = case
    res = _run([case], max_iteration=30)
    p2p = REG.refine_batch([src], [tgt], None, D, max_iteration=30)
    a, b = PR.worst_displacement(src, res.matrices[0], T_gt), PR.worst_displacement(src, p2p.matrices[0], T_gt)
    print(f"epsilon = 1: {res.iterations[0]} updates, worst point {a:.4e} m; point-to-point: {p2p.iterations[0]} updates, {b:.4e} m")
    assert 2 <= res.iterations[0] < 30 and 2 <= p2p.iterations[0] < 30
    assert abs(a - b) <= 1e-4


# --- degenerate and poisoned input ---------------------------------------------------------------------------------------
def test_zero_and_nan_covariances_stop_the_pair_at_once(cuda):
    src, tgt, cs, ct, start, T_gt = GR.case("offset")
    clean = (src, tgt, cs, ct, start)
    want = _run([clean])
    assert want.iterations[0] >= 2
    corr0 = IR.evaluate(src, tgt, start, D)[0]
    assert (corr0 >= 0).all()
    nan_t = ct.copy()
    nan_t[corr0[17], 4] = np.nan
    nan_s = cs.copy()
    nan_s[1199] = np.nan
    for name, dirty in (("zero", (src, tgt, np.zeros_like(cs), np.zeros_like(ct), start)), ("nan target", (src, tgt, cs, nan_t, start)),
                        ("nan source", (src, tgt, nan_s, ct, start))):
        res = _run([clean, dirty, clean], trace=True)
        tr, _ = _check_steps(res, 1, *dirty)
        assert res.iterations[1] == 0 and res.matrices[1].tobytes() == start.tobytes(), name
        assert res.counts[1] == len(src) and res.fitness[1] == 1.0 and res.inlier_rmse[1] > 0, name
        assert not np.isfinite(tr["sums27"][0]).any() if name == "zero" else not np.isfinite(tr["sums27"][0]).all(), name
        assert _five(res, 0) == _five(want, 0) == _five(res, 2), name         # the clean pairs beside it


def test_a_nan_row_that_is_nobody_s_correspondence_changes_nothing(cuda):
    src, tgt, cs, ct, start, T_gt = GR.case("offset")
    far_t = np.concatenate([tgt, np.array([[3.0, 3.0, 3.0]], np.float32)])
    far_s = np.concatenate([src, np.array([[-3.0, -3.0, -3.0]], np.float32)])
    iso = np.array([[1.0, 0, 0, 1, 0, 1]])
    clean = (far_s, far_t, np.concatenate([cs, iso]), np.concatenate([ct, iso]), start)
    run = GR.icp(*clean, D, max_iteration=MI)
    for Tk, _, _ in run[5]:
        corr = IR.evaluate(far_s, far_t, Tk, D)[0]
        assert corr[-1] == -1 and (corr != len(tgt)).all()
        p = IR.move(far_s, Tk).astype(np.float64)
        assert np.sqrt(((p[:-1] - far_t[-1]) ** 2).sum(1)).min() > 2 * D and np.sqrt(((p[-1] - far_t) ** 2).sum(1)).min() > 2 * D
    want = _run([clean], trace=True)
    assert want.iterations[0] == run[4] >= 2
    for bad in (np.nan, np.inf):
        dirty = (far_s, far_t, np.concatenate([cs, np.full((1, 6), bad)]), np.concatenate([ct, np.full((1, 6), bad)]), start)
        got = _run([dirty], trace=True)
        assert _five(got, 0) == _five(want, 0)
        a, b = _host(got.trace, 0), _host(want.trace, 0)
        for key in ("T", "counts", "sums", "sums27", "corr"):
            assert a[key].tobytes() == b[key].tobytes(), key


def test_empty_clouds_and_a_nan_start(cuda):
    src, tgt, cs, ct, start, T_gt = GR.case("offset")
    e3, e6 = np.zeros((0, 3), np.float32), np.zeros((0, 6))
    cases = [(e3, tgt, e6, ct, T_gt), (src, e3, cs, e6, T_gt), (src, tgt, cs, ct, np.eye(4)), (src, tgt, cs, ct, np.eye(4))]
    clean = _run(cases)
    for b in range(2):
        assert np.array_equal(clean.matrices[b], T_gt), b
        assert clean.fitness[b] == 0 and clean.inlier_rmse[b] == 0 and clean.counts[b] == 0 and clean.iterations[b] == 0, b
    assert clean.iterations[2] >= 2 and _five(clean, 2) == _five(clean, 3)
    bad = np.eye(4)
    bad[1, 2] = np.nan
    cases[2] = (src, tgt, cs, ct, bad)
    res = _run(cases)
    assert np.isnan(res.matrices[2]).all() and np.isnan(res.fitness[2]) and res.counts[2] == -1 and res.iterations[2] == -1
    for b in (0, 1, 3):
        assert _five(res, b) == _five(clean, b), b


def _c_entry(src, tgt, cs, ct, n_max=None, mi=MI):
    """One pair through pcrcg_gicp_batch from the identity -> (transform [16], stats [4]) on the host."""
    L = _lib.lib()
    dev = torch.device("cuda")
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    n, m = len(src), len(tgt)
    offs = torch.tensor([0, n, 0, m, m], dtype=torch.int32, device=dev)
    gbytes = L.pcrcg_cellgrid_ws_bytes(m, 1)
    grid = torch.empty(gbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.pcrcg_cellgrid_build(t.data_ptr(), m, offs[4:].data_ptr(), 1, D, grid.data_ptr(), gbytes, st), "grid")
    wsb = L.pcrcg_gicp_batch_ws_bytes(1, n, m, mi)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.full((20,), -7.0, dtype=torch.float64, device=dev)
    csd, ctd = torch.from_numpy(np.ascontiguousarray(cs)).to(dev), torch.from_numpy(np.ascontiguousarray(ct)).to(dev)
    _lib.check(L.pcrcg_gicp_batch(s.data_ptr(), offs.data_ptr(), n, n if n_max is None else n_max, offs[2:].data_ptr(), m,
                                  grid.data_ptr(), None, 1, D, mi, 1e-6, 1e-6, csd.data_ptr(), ctd.data_ptr(), out.data_ptr(),
                                  out[16:].data_ptr(), None, ws.data_ptr(), wsb, st), "pcrcg_gicp_batch")
    h = out.cpu().numpy()
    return h[:16], h[16:]


def test_a_pair_longer_than_n_max_gets_nan_and_the_c_entry_is_the_python_entry(cuda):
    src, tgt, cs, ct, start, T_gt = GR.case("offset")
    T, stats = _c_entry(src, tgt, cs, ct, n_max=len(src) - 1)
    assert np.isnan(T).all() and np.isnan(stats).all()
    T, stats = _c_entry(src, tgt, cs, ct)
    py = _run([(src, tgt, cs, ct, start)])
    assert T.tobytes() == py.matrices[0].tobytes() and stats[3] == py.iterations[0] >= 2 and stats[2] == py.counts[0]


# --- batching ------------------------------------------------------------------------------------------------------------
RAGGED = ((0, 50), (1, 40), (64, 100), (700, 513), (1200, 1500))


@pytest.fixture(scope="module")
def ragged():
    """Five pairs of RAGGED's lengths: samples of the corner surface under the small pose with 1 mm noise, exact-surface
    normals' covariances -> a list of (src, tgt, C_s, C_t, start)."""
    out = []
    T = PR.small_pose()
    for i, (n, m) in enumerate(RAGGED):
        ps, pt = PR.corner(500 + i, n), PR.corner(600 + i, m)
        rng = np.random.RandomState(700 + i)
        tgt = pt @ T[:3, :3].T + T[:3, 3] + 0.001 * rng.randn(m, 3)
        cs = GR.covariances_from_normals(PR.corner_normals(ps), GR.EPSILON).reshape(n, 6)
        ct = GR.covariances_from_normals(PR.corner_normals(pt) @ T[:3, :3].T, GR.EPSILON)
        out.append((ps.astype(np.float32).reshape(n, 3), tgt.astype(np.float32), cs, ct, np.eye(4)))
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
        single = REG.generalized_icp(ragged[b][0], ragged[b][1], ragged[b][4], D, src_covariances=GR.unpack(ragged[b][2]),
                                     tgt_covariances=GR.unpack(ragged[b][3]), max_iteration=MI)
        assert (single.matrix.tobytes(), single.iterations) == (alone.matrices[0].tobytes(), alone.iterations[0])
    assert batch.iterations[0] == 0 and batch.counts[0] == 0 and batch.matrices[0].tobytes() == np.eye(4).tobytes()
    assert batch.iterations[1] == 0 and batch.counts[1] <= 1
    assert (batch.iterations[2:] >= 2).all()
    # numpy, device and mixed inputs
    dev = torch.device("cuda", torch.cuda.current_device())
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    forms = {"device": lambda b, x: on(x), "mixed": lambda b, x: on(x) if b % 2 else x}
    for name, f in forms.items():
        got = REG.generalized_icp_batch([f(b, c[0]) for b, c in enumerate(ragged)], [f(b + 1, c[1]) for b, c in enumerate(ragged)],
                                        on(np.stack([c[4] for c in ragged])) if name == "device" else None, D, max_iteration=MI,
                                        src_covariances=[f(b, GR.unpack(c[2])) for b, c in enumerate(ragged)],
                                        tgt_covariances=[f(b + 1, GR.unpack(c[3])) for b, c in enumerate(ragged)])
        assert [_five(got, b) for b in range(5)] == [_five(batch, b) for b in range(5)], name


def test_a_fast_global_registration_result_as_the_start_adds_no_read(cuda):
    src, tgt, cs, ct, start, T_gt = GR.case("offset")
    pairs = np.stack([np.arange(0, 1200, 7), np.arange(0, 1200, 7)], 1)
    fgr = REG.fast_global_registration_batch([src, src], [tgt, tgt], maximum_correspondence_distance=0.05,
                                             correspondences=[pairs, pairs], seeds=[3, 4])
    assert isinstance(fgr, REG.FastGlobalRegistrationResult)
    reads = REG.D2H_READS
    res = _run_init([(src, tgt, cs, ct)] * 2, fgr)
    assert REG.D2H_READS == reads + 1
    by_array = _run_init([(src, tgt, cs, ct)] * 2, fgr.matrices)
    for b in range(2):
        assert _five(res, b) == _five(by_array, b)
        assert PR.worst_displacement(src, res.matrices[b], T_gt) < 1e-6


def _run_init(cases, init):
    return REG.generalized_icp_batch([c[0] for c in cases], [c[1] for c in cases], init, D, max_iteration=MI,
                                     src_covariances=[GR.unpack(c[2]) for c in cases],
                                     tgt_covariances=[GR.unpack(c[3]) for c in cases])


# --- the three ways to give a side its covariances -----------------------------------------------------------------------
def test_covariances_normals_and_a_radius_agree_bit_for_bit(cuda, ragged):
    srcs, tgts = [c[0] for c in ragged[2:]], [c[1] for c in ragged[2:]]
    kw = dict(max_iteration=MI)
    reads = REG.D2H_READS
    inside = REG.generalized_icp_batch(srcs, tgts, None, D, normal_radius=R_NORMAL, trace=True, **kw)
    assert REG.D2H_READS == reads + 1
    ns, nt = REG.estimate_normals_batch(srcs, R_NORMAL, 30), REG.estimate_normals_batch(tgts, R_NORMAL, 30)
    cs, ct = [REG.covariances_from_normals(x) for x in ns], [REG.covariances_from_normals(x) for x in nt]
    for b in range(3):
        assert torch.equal(inside.trace["src_covariances"][b], cs[b]) and torch.equal(inside.trace["tgt_covariances"][b], ct[b])
    full = lambda c: torch.from_numpy(GR.unpack(c.cpu().numpy())).cuda()
    runs = [REG.generalized_icp_batch(srcs, tgts, None, D, src_normals=ns, tgt_normals=nt, **kw),
            REG.generalized_icp_batch(srcs, tgts, None, D, src_covariances=[full(c) for c in cs],
                                      tgt_covariances=[full(c) for c in ct], **kw),
            REG.generalized_icp_batch(srcs, tgts, None, D, src_normals=[x.cpu().numpy() for x in ns], normal_radius=R_NORMAL, **kw),
            REG.generalized_icp_batch(srcs, tgts, None, D, tgt_covariances=[full(c) for c in ct], normal_radius=R_NORMAL,
                                      pairs_per_call=2, **kw)]
    for b in range(3):
        for r in runs:
            assert _five(r, b) == _five(inside, b), b
    assert (inside.iterations[1:] >= 2).all() and (inside.iterations >= 1).all()
    # epsilon reaches the builder: another epsilon, other covariances
    other = REG.generalized_icp_batch(srcs, tgts, None, D, normal_radius=R_NORMAL, epsilon=1e-2, trace=True, **kw)
    assert torch.equal(other.trace["tgt_covariances"][0], REG.covariances_from_normals(nt[0], 1e-2))


def test_the_tester_dispatches_to_the_generalized_entry(cuda):
    from pcrcg_amd import tester
    from . import ransac_ref as RR
    records = []
    for seed in (31, 32):
        src, tgt, f, g, T_gt = RR.registration_pair(seed, n=1200, outliers=0.5)
        n = len(src)
        records.append({"pcd": torch.from_numpy(np.concatenate([src, tgt])), "feats": torch.from_numpy(np.concatenate([f, g])),
                        "overlaps": torch.ones(2 * n), "saliency": torch.rand(2 * n, generator=torch.Generator().manual_seed(seed)) + 0.1,
                        "len_src": n, "rot": torch.from_numpy(T_gt[:3, :3].astype(np.float32)),
                        "trans": torch.from_numpy(T_gt[:3, 3:].astype(np.float32))})
    kw = dict(n_points=500, distance_threshold=0.05, ransac_n=3, seeds=[1, 2])
    np.random.seed(0)
    start = REG.register_batch(*tester._sample_records(records, 500), 0.05, 3, seeds=[1, 2])
    np.random.seed(0)
    fine = tester.register_records(records, refine=0.05, icp_estimation="generalized", normal_radius=0.1, **kw)
    np.random.seed(0)
    fine2, _ = tester.evaluate_records(records, refine=0.05, icp_estimation="generalized", normal_radius=0.1, **kw)
    direct = REG.generalized_icp_batch([r["pcd"][:r["len_src"]] for r in records], [r["pcd"][r["len_src"]:] for r in records],
                                       start, 0.05, normal_radius=0.1)
    for b in range(2):
        assert fine[b].tobytes() == fine2[b].tobytes() == direct.matrices[b].tobytes()
    assert (direct.iterations >= 1).all()
