"""GPU: point-to-plane ICP (csrc/icp.hip: pcrcg_icp_batch_ex, k_icp_evaluate<1>, k_icp_update<1>; csrc/smallsolve.h) on the paths
tests/test_icp_plane_gpu.py does not reach: ill-conditioned systems (clouds far from the origin, a nearly planar pair), the
pivot rule refusing an update, the 28-term partial-sum slots around 512-row boundaries, the stop rules, the strict distance
threshold, a start outside the grid, the untraced launch, normals that are NaN, inf, zero or fallback rows, and normals
estimated in the call for a ragged batch.  Every trace is still checked step by step against tests/icp_plane_ref.py
(test_icp_plane_gpu._check_steps); tests/test_icp_plane_cpu.py::test_the_cases_are_what_they_claim checks on the CPU that
the cases are what they are taken for.

Ill-conditioned pairs go through _check_steps_split, which separates what the device adds to the error from what the
conditioning does to ANY float64 solve:
  1. correspondences and counts exact, the 27 sums within 1e-12 x the sums of the terms' absolute values;
  2. T_k+1 against step_from_sums(the device's own 27 sums, T_k) -- the same solver on the same numbers -- within
     1e-12 max(1, max|T_k|, max|x|): about a hundred float64 roundings on values of that size and one or two ulp in sin / cos
     (tests/test_smallsolve_cpu.py: the header compiled for the host agrees with numpy bit for bit);
  3. T_k+1 against the np.longdouble solve of the RESTATED sums within 1e-13 cond(A) max|x| -- the project's 1e-13 cond(A)
     (_check_steps with max_cond=None) scaled by the size of the solution -- plus 4e-15 max(1, max|T_k|, max|x|) for forming
     delta T_k from x in float64 (FORM below: 36 roundings, counted there).  That part does not shrink with x: at the last
     update of a converged pair |x| is 1e-9 and cond(A) 28, so 1e-13 cond(A) max|x| alone is 3e-21, below one ulp of T.

The ladder (offset_pair: the 1 200-point corner cloud and its image under a 0.4 degree / 1.8 cm pose, both moved s metres along
every axis; d = 0.15, restated normals at r = 0.12 / 30, at most 10 updates).  Restatement, then device (MI355X):

  s (m)   cond(A) at T_0   lowest pivot ratio   updates   worst point after (m)   largest |T_k+1| difference: 2, 3
  0       2.8e1            1.3e-1               3 / 3     1.0e-9 / 1.0e-9         1.1e-16, 2.0e-16
  10      8.4e5            2.8e-6               4 / 4     6.0e-7 / 6.0e-7         6.9e-18, 2.0e-13
  100     7.0e9            3.4e-10              5 / 5     5.4e-6 / 5.4e-6         2.8e-17, 6.2e-10
  1000    6.8e13           3.5e-14              0 / 0     0.02 (the start)        (no update: the rule refuses at T_0)

The device took the restatement's decisions on every rung and ended at the same worst point to the four digits printed.
Comparison 2 never exceeded 1.2e-4 of its bound, comparison 3 2.6e-2 (at s = 0, where the bound is the 4e-15 of forming
delta T_k; at s = 100: 6.2e-10 against a bound of 5.3e-4, the conditioning's share).  The two nearly planar pairs (lowest pivot ratios 5.7e-9 and 3.2e-11; the second is the one a rule
of 1e-10 would refuse) measured 3.5e-14 and 2.1e-13 in comparison 3.
"""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import icp_plane_ref as PR
from . import icp_ref as IR
from . import normals_ref as NR
from .test_icp_edges_gpu import H, _threshold_clouds
from .test_icp_plane_gpu import D, MI, PLANE, R_NORMAL, _check_steps, _host

pytestmark = pytest.mark.gpu

# What forming delta(x) T_k in float64 may add to comparison 3, over the size of the entries (u = 2^-53 = 1.1e-16): sin and
# cos within 2 u each; an entry of Rz Ry Rx is a product of three of them (6 u and 2 roundings) or a sum of two such (one
# more): 9 u; a row of delta times a column of T_k is up to four products (one rounding each) added in turn (three more), on
# terms whose absolute values add up to at most (sqrt(3) + 1) size (a unit row, and the step's translation): 13 u x 2.74 =
# 36 u = 4e-15.  It does not shrink with x: the last updates of a converged pair have |x| of 1e-9 and T entries of order 1.
FORM = 4e-15


def _check_steps_split(res, b, src, tgt, nrm, T0, d=D, mi=MI):
    """Pair b of a traced result, one step at a time, with the three comparisons of the module's docstring -> (its host trace,
    the largest error over its bound of comparisons 2 and 3)."""
    tr = _host(res.trace, b)
    n = len(src)
    iters = int(res.iterations[b])
    assert 0 <= iters <= mi
    assert np.array_equal(tr["T"][0], np.asarray(T0, np.float64))
    can_update, worst2, worst3 = {}, 0.0, 0.0
    for k in range(iters + 1):
        Tk = tr["T"][k]
        corr, _, count, total = IR.evaluate(src, tgt, Tk, d)
        got = tr["corr"][k].astype(np.int64)
        assert (got == corr).all(), (k, np.flatnonzero(got != corr)[:5])
        assert tr["counts"][k] == count, k
        assert abs(tr["sums"][k] - total) <= 1e-12 * max(abs(total), 1e-300), k
        want, mag = PR.sums27(src, tgt, nrm, Tk, got)
        err = np.abs(tr["sums27"][k] - want)
        assert (err <= 1e-12 * mag).all(), (k, err, mag)
        same = PR.step_from_sums(tr["sums27"][k], Tk)
        can_update[k] = count >= PR.MIN_COUNT and same is not None
        assert can_update[k] == (PR.update(src, tgt, nrm, Tk, got)[0] is not None), k     # no decision hangs on the sums' last bits
        if k < iters:
            assert same is not None, k
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
            print(f"step {k}: count {count}, sums27 error / bound {float((err / np.maximum(mag, 1e-300)).max() / 1e-12):.2e}, "
                  f"cond {cond:.3e}, lowest pivot ratio {PR.pivot_ratios(A).min():.2e}, max|x| {np.abs(x).max():.2e}, "
                  f"same sums {e2:.2e} (bound {b2:.2e}), longdouble {e3:.2e} (bound {b3:.2e})")
            worst2, worst3 = max(worst2, e2 / b2), max(worst3, e3 / b3)
            assert e2 <= b2 and e3 <= b3, (k, e2, b2, e3, b3)
    assert IR.stop_iteration(tr["counts"], tr["sums"], n, lambda k: can_update[k], mi) == iters
    assert (tr["counts"][iters + 1:] == -1).all() and np.isnan(tr["T"][iters + 1:]).all()
    assert np.isnan(tr["sums27"][iters + 1:]).all() and np.isnan(tr["sums"][iters + 1:]).all()
    fit, rmse = IR.statistics(int(tr["counts"][iters]), float(tr["sums"][iters]), n)
    assert np.array_equal(res.matrices[b], tr["T"][iters])
    assert res.fitness[b] == fit and res.inlier_rmse[b] == rmse and res.counts[b] == tr["counts"][iters]
    return tr, (float(worst2), float(worst3))


def _five(res, b):
    """The five outputs of pair b, as bytes and numbers that compare bit for bit."""
    return (res.matrices[b].tobytes(), np.float64(res.fitness[b]).tobytes(), np.float64(res.inlier_rmse[b]).tobytes(),
            int(res.counts[b]), int(res.iterations[b]))


# --- far from the origin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", PR.LADDER)
def test_the_ladder_updates_as_the_restatement_does(cuda, shift):
    src, tgt, T_gt, nrm, run = PR.ladder_case(shift)
    res = REG.refine_batch([src], [tgt], None, PR.LADDER_D, max_iteration=PR.LADDER_MI, trace=True, tgt_normals=[nrm], **PLANE)
    tr, worst = _check_steps_split(res, 0, src, tgt, nrm, np.eye(4), d=PR.LADDER_D, mi=PR.LADDER_MI)
    got = PR.worst_displacement(src, res.matrices[0], T_gt)
    want = PR.worst_displacement(src, run[0], T_gt)
    print(f"s = {shift}: updates {res.iterations[0]} (restatement {run[4]}), worst point {got:.3e} m (restatement {want:.3e} m), "
          f"largest error / bound: same sums {worst[0]:.2e}, longdouble {worst[1]:.2e}")
    assert res.iterations[0] >= 2 and res.fitness[0] == 1.0
    assert got <= max(3.0 * want, 1e-9)


def test_a_thousand_metres_out_the_rule_refuses_the_first_update(cuda):
    src, tgt, T_gt, nrm, run = PR.ladder_case(PR.FAR)
    start = np.eye(4)
    res = REG.refine_batch([src], [tgt], start[None], PR.LADDER_D, max_iteration=PR.LADDER_MI, trace=True, tgt_normals=[nrm],
                           **PLANE)
    tr, _ = _check_steps_split(res, 0, src, tgt, nrm, start, d=PR.LADDER_D, mi=PR.LADDER_MI)
    assert res.iterations[0] == 0 and res.matrices[0].tobytes() == start.tobytes()
    assert run[4] == 0 and (res.fitness[0], res.inlier_rmse[0], res.counts[0]) == (run[1], run[2], run[3])
    assert res.counts[0] == len(src) and PR.step_from_sums(tr["sums27"][0], start) is None
    ratios = PR.pivot_ratios(PR.system(tr["sums27"][0])[0])
    print("s = 1000: the device's pivot ratios", ratios, "worst point", PR.worst_displacement(src, res.matrices[0], T_gt))
    assert ratios.min() <= 1e-13


@pytest.mark.parametrize("tilt", sorted(PR.NEAR_PLANE_TILTS, reverse=True))
def test_a_nearly_planar_pair_is_not_refused(cuda, tilt):
    low, high = PR.NEAR_PLANE_TILTS[tilt]
    src, tgt, nrm, start = PR.near_plane_pair(tilt=tilt)
    res = REG.refine_batch([src], [tgt], start[None], D, max_iteration=MI, trace=True, tgt_normals=[nrm], **PLANE)
    tr, worst = _check_steps_split(res, 0, src, tgt, nrm, start)
    ratios = PR.pivot_ratios(PR.system(tr["sums27"][0])[0])
    print("near plane, tilt", tilt, "updates", res.iterations[0], "pivot ratios at T_0", ratios, "largest error / bound", worst)
    assert res.iterations[0] >= 1 and low <= ratios.min() <= high
    assert res.fitness[0] == 1.0 and np.abs(res.matrices[0] - np.eye(4)).max() < 1e-5


# --- sizes: the 28-term slots ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized():
    return [PR.sized_pair(i, n) for i, n in enumerate(PR.SIZES)]


def _sized_args(sized, idx):
    return ([sized[i][0] for i in idx], [sized[i][1] for i in idx], np.stack([sized[i][3] for i in idx]), D)


def test_every_size_in_one_batch(cuda, sized):
    idx = list(range(len(PR.SIZES)))
    kw = dict(max_iteration=MI, **PLANE)
    batch = REG.refine_batch(*_sized_args(sized, idx), trace=True, tgt_normals=[sized[i][2] for i in idx], **kw)
    two = REG.refine_batch(*_sized_args(sized, idx), pairs_per_call=2, tgt_normals=[sized[i][2] for i in idx], **kw)
    for i, n in enumerate(PR.SIZES):
        src, tgt, nrm, start = sized[i]
        tr = _check_steps(batch, i, src, tgt, nrm, start, max_cond=None)
        assert tr["counts"][0] == n
        alone = REG.refine_batch(*_sized_args(sized, [i]), tgt_normals=[nrm], **kw)
        assert _five(batch, i) == _five(alone, 0) == _five(two, i), n
        if n < PR.MIN_COUNT:
            assert batch.iterations[i] == 0 and batch.matrices[i].tobytes() == start.tobytes(), n
        else:
            assert batch.iterations[i] >= 1, n
    # the same pairs in another order: every pair's first slot moves, its bits do not
    order = [8, 0, 6, 2, 4, 7, 1, 5, 3]
    shuffled = REG.refine_batch(*_sized_args(sized, order), tgt_normals=[sized[i][2] for i in order], **kw)
    for pos, i in enumerate(order):
        assert _five(shuffled, pos) == _five(batch, i), PR.SIZES[i]


def test_the_untraced_launch_equals_the_traced_one(cuda, sized):
    idx = list(range(len(PR.SIZES)))
    kw = dict(max_iteration=MI, tgt_normals=[sized[i][2] for i in idx], **PLANE)
    traced = REG.refine_batch(*_sized_args(sized, idx), trace=True, **kw)
    plain = REG.refine_batch(*_sized_args(sized, idx), **kw)
    assert plain.trace is None
    for i in idx:
        assert _five(traced, i) == _five(plain, i), PR.SIZES[i]
    assert torch.equal(traced.transformations, plain.transformations)
    assert (plain.iterations[2:] >= 1).all()


# --- the stop rules ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corner():
    src, tgt, T_gt = PR.corner_pair()
    return src, tgt, T_gt, NR.estimate(tgt, R_NORMAL, 30)["normals"]


@pytest.fixture(scope="module")
def corner_long(cuda, corner):
    """The corner pair with both bounds 0 and a cap of 6: only the cap stops it."""
    src, tgt, _, nrm = corner
    return REG.refine_batch([src], [tgt], None, D, max_iteration=6, relative_fitness=0.0, relative_rmse=0.0, trace=True,
                            tgt_normals=[nrm], **PLANE)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_the_iteration_cap_stops_the_loop(cuda, corner, corner_long, cap):
    src, tgt, _, nrm = corner
    res = REG.refine_batch([src], [tgt], None, D, max_iteration=cap, trace=True, tgt_normals=[nrm], **PLANE)
    assert res.iterations[0] == cap
    # a trace has max_iteration + 1 rows, so THIS call has none beyond its cap to leave untouched; that rows past a stop keep
    # their fill is checked where there are some (test_the_default_thresholds_stop_before_the_cap, _check_steps), and that
    # the cap changes nothing before it by the prefix of the longer run below
    tr = _check_steps(res, 0, src, tgt, nrm, np.eye(4), mi=cap)
    assert tr["T"].shape[0] == cap + 1 and res.matrices[0].tobytes() == tr["T"][cap].tobytes()
    assert (tr["counts"] >= PR.MIN_COUNT).all() and np.isfinite(tr["T"]).all() and np.isfinite(tr["sums27"]).all()
    # the same steps as the first `cap` of a longer run, bit for bit; that run's trace ends at ITS cap
    long = _host(corner_long.trace, 0)
    assert corner_long.iterations[0] == 6 and tr["T"].tobytes() == long["T"][:cap + 1].tobytes()
    assert tr["sums27"].tobytes() == long["sums27"][:cap + 1].tobytes()


def test_the_default_thresholds_stop_before_the_cap(cuda, corner, corner_long):
    src, tgt, _, nrm = corner
    res = REG.refine_batch([src], [tgt], None, D, trace=True, tgt_normals=[nrm], **PLANE)         # max_iteration = 30
    tr = _check_steps(res, 0, src, tgt, nrm, np.eye(4), mi=30)
    k = int(res.iterations[0])
    assert 2 <= k < 6 and tr["T"].shape[0] == 31
    # it was the convergence test: another update was there to be made, and the run without bounds made it
    assert PR.update(src, tgt, nrm, tr["T"][k], tr["corr"][k].astype(np.int64))[0] is not None
    assert _host(corner_long.trace, 0)["T"][:k + 1].tobytes() == tr["T"][:k + 1].tobytes()
    # rows past the stop keep their fill
    assert (tr["counts"][k + 1:] == -1).all() and np.isnan(tr["T"][k + 1:]).all() and np.isnan(tr["sums27"][k + 1:]).all()
    assert (tr["corr"][k + 1:] == -2).all()


def test_a_start_that_moves_every_point_out_of_the_grid(cuda, corner, sized):
    src, tgt, _, nrm = corner
    S = np.eye(4)
    S[0, 3] = 1e9
    assert IR.grid_rejects(IR.move(src, S), D).all()
    res = REG.refine_batch([src], [tgt], S[None], D, max_iteration=MI, trace=True, tgt_normals=[nrm], **PLANE)
    _check_steps(res, 0, src, tgt, nrm, S)
    assert res.counts[0] == 0 and res.iterations[0] == 0 and res.fitness[0] == 0.0 and res.inlier_rmse[0] == 0.0
    assert res.matrices[0].tobytes() == S.tobytes() and (_host(res.trace, 0)["corr"][0] == -1).all()
    a, b = sized[6], sized[8]                                         # 513 and 1025 rows on either side of it
    batch = REG.refine_batch([a[0], src, b[0]], [a[1], tgt, b[1]], np.stack([a[3], S, b[3]]), D, max_iteration=MI,
                             tgt_normals=[a[2], nrm, b[2]], **PLANE)
    assert _five(batch, 1) == _five(res, 0)
    for pos, p in ((0, a), (2, b)):
        alone = REG.refine_batch([p[0]], [p[1]], p[3][None], D, max_iteration=MI, tgt_normals=[p[2]], **PLANE)
        assert _five(batch, pos) == _five(alone, 0) and alone.iterations[0] >= 1


def test_the_threshold_is_strict(cuda):
    src, exact, _, _, own = _threshold_clouds()
    rng = np.random.RandomState(9)
    nrm = rng.randn(len(exact), 3)
    nrm[::5] = [0.0, 0.0, 1.0]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    above = float(np.nextafter(np.float32(H), np.float32(np.inf)))      # one fp32 step: (float)(d d) is above 2^-6
    assert len(src) >= PR.MIN_COUNT and np.float32(above * above) > np.float32(H * H) == H * H
    at = REG.refine_batch([src], [exact], None, H, max_iteration=2, trace=True, tgt_normals=[nrm], **PLANE)
    tr = _check_steps(at, 0, src, exact, nrm, np.eye(4), d=H, mi=2, max_cond=None)
    assert (tr["corr"][0] == -1).all() and at.counts[0] == 0 and at.iterations[0] == 0 and at.fitness[0] == 0.0
    # one float64 step above H is still H to the kernel: the threshold is (float)(d d), and that product rounds to 2^-6
    barely = float(np.nextafter(H, np.inf))
    assert barely > H and np.float32(barely * barely) == np.float32(H * H)
    same = REG.refine_batch([src], [exact], None, barely, max_iteration=2, tgt_normals=[nrm], **PLANE)
    assert _five(same, 0) == _five(at, 0)
    over = REG.refine_batch([src], [exact], None, above, max_iteration=2, trace=True, tgt_normals=[nrm], **PLANE)
    tr = _check_steps(over, 0, src, exact, nrm, np.eye(4), d=above, mi=2, max_cond=None)
    assert (tr["corr"][0] == own).all() and tr["counts"][0] == len(src) and over.iterations[0] >= 1


# --- normals -----------------------------------------------------------------------------------------------------------
def test_a_bad_normal_nobody_reads_changes_no_bit(cuda, corner):
    src, tgt, _, nrm = corner
    far = np.concatenate([tgt, np.array([[3.0, 3.0, 3.0]], np.float32)])
    clean = np.concatenate([nrm, [[0.0, 0.0, 1.0]]])
    run = PR.icp(src, far, clean, np.eye(4), D, max_iteration=MI)
    for Tk, _, _ in run[5]:
        gap = np.sqrt(((IR.move(src, Tk).astype(np.float64) - far[-1].astype(np.float64)) ** 2).sum(1)).min()
        assert gap > 2 * D
    want = REG.refine_batch([src], [far], None, D, max_iteration=MI, trace=True, tgt_normals=[clean], **PLANE)
    assert want.iterations[0] == run[4] >= 2
    for bad in (np.nan, np.inf):
        dirty = clean.copy()
        dirty[-1] = bad
        got = REG.refine_batch([src], [far], None, D, max_iteration=MI, trace=True, tgt_normals=[dirty], **PLANE)
        assert _five(got, 0) == _five(want, 0)
        a, b = _host(got.trace, 0), _host(want.trace, 0)
        for key in ("T", "counts", "sums", "sums27", "corr"):
            assert a[key].tobytes() == b[key].tobytes(), key


@pytest.fixture(scope="module")
def resampled():
    """The resampled corner pair, its restated normals, the restatement's correspondences per step, and a target that is
    first matched at step `first` >= 1 -> src, tgt, nrm, j, first."""
    src, tgt, _ = PR.corner_pair(m=2000, noise=0.002)
    nrm = NR.estimate(tgt, R_NORMAL, 30)["normals"]
    run = PR.icp(src, tgt, nrm, np.eye(4), D, max_iteration=MI)
    seen = [set(IR.evaluate(src, tgt, Tk, D)[0].tolist()) - {-1} for Tk, _, _ in run[5]]
    assert run[4] >= 2
    late = sorted(seen[1] - seen[0])
    assert late, "no target is first matched at the second evaluation"
    return src, tgt, nrm, late[0], 1


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_bad_normal_stops_the_pair_where_it_is_first_matched(cuda, corner, resampled, bad):
    src, tgt, nrm, j, first = resampled
    c_src, c_tgt, _, c_nrm = corner
    clean = REG.refine_batch([src, c_src], [tgt, c_tgt], None, D, max_iteration=MI, trace=True, tgt_normals=[nrm, c_nrm], **PLANE)
    ctr = _host(clean.trace, 0)
    assert clean.iterations[0] > first
    assert j not in set(ctr["corr"][0].tolist()) and j in set(ctr["corr"][first].tolist())
    for row in (np.full(3, bad), np.array([nrm[j, 0], bad, nrm[j, 2]])):
        dirty = nrm.copy()
        dirty[j] = row
        got = REG.refine_batch([c_src, src], [c_tgt, tgt], None, D, max_iteration=MI, trace=True, tgt_normals=[c_nrm, dirty],
                               **PLANE)
        tr = _host(got.trace, 1)
        assert got.iterations[1] == first
        assert tr["T"][:first + 1].tobytes() == ctr["T"][:first + 1].tobytes()
        assert tr["corr"][:first + 1].tobytes() == ctr["corr"][:first + 1].tobytes()
        assert got.matrices[1].tobytes() == ctr["T"][first].tobytes()
        fit, rmse = IR.statistics(int(ctr["counts"][first]), float(ctr["sums"][first]), len(src))
        assert np.isfinite([fit, rmse]).all() and rmse > 0
        assert (got.fitness[1], got.inlier_rmse[1], got.counts[1]) == (fit, rmse, ctr["counts"][first])
        assert not np.isfinite(tr["sums27"][first]).all() and np.isfinite(tr["sums27"][:first]).all()
        assert (tr["counts"][first + 1:] == -1).all() and np.isnan(tr["T"][first + 1:]).all()
        want = PR.icp(src, tgt, dirty, np.eye(4), D, max_iteration=MI)
        assert want[4] == first
        assert _five(got, 0) == _five(clean, 1) and clean.iterations[1] >= 2       # the clean pair beside it


def test_zero_normals_stop_at_the_start(cuda, corner):
    src, tgt, T_gt, nrm = corner
    start = PR.small_pose() @ T_gt
    res = REG.refine_batch([src, src], [tgt, tgt], np.stack([start, start]), D, max_iteration=MI, trace=True,
                           tgt_normals=[np.zeros_like(nrm), nrm], **PLANE)
    tr = _check_steps(res, 0, src, tgt, np.zeros_like(nrm), start)
    assert res.iterations[0] == 0 and res.matrices[0].tobytes() == start.tobytes() and res.counts[0] == len(src)
    assert (tr["sums27"][0] == 0).all() and res.fitness[0] == 1.0 and res.inlier_rmse[0] > 0
    assert res.iterations[1] >= 1


def _isolated_pair():
    """The corner cloud and 12 points more than 0.3 m from it and from each other, under the small pose: the restated normals
    of the 12 are the fallback row (0, 0, 1), and every one of them is some source's correspondence."""
    lattice = np.stack(np.meshgrid(np.arange(3), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([PR.corner(0, 1200), 1.4 + 0.4 * lattice])
    T = PR.small_pose()
    return pts.astype(np.float32), (pts @ T[:3, :3].T + T[:3, 3]).astype(np.float32), T


def test_fallback_normals_are_rows_like_any_other(cuda):
    src, tgt, T_gt = _isolated_pair()
    est = NR.estimate(tgt, R_NORMAL, 30)
    nrm = est["normals"]
    assert est["fallback"].sum() == 12 and est["fallback"][-12:].all() and (nrm[-12:] == [0.0, 0.0, 1.0]).all()
    res = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, trace=True, tgt_normals=[nrm], **PLANE)
    tr = _check_steps(res, 0, src, tgt, nrm, np.eye(4))
    assert (tr["corr"][0][-12:] == np.arange(1200, 1212)).all() and res.iterations[0] >= 2 and res.fitness[0] == 1.0
    inside = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, trace=True, normal_radius=R_NORMAL, **PLANE)
    got = inside.trace["normals"][0].cpu().numpy()
    assert (got[-12:] == [0.0, 0.0, 1.0]).all()


RAGGED_M = (0, 1, 2, 3, 64, 700)


def test_normals_estimated_in_the_call_for_a_ragged_batch(cuda):
    rng = np.random.RandomState(21)
    T = PR.small_pose()
    srcs, tgts = [], []
    for i, m in enumerate(RAGGED_M):
        surface = PR.corner(400 + i, max(m, 400))
        if m <= 3:      # the targets' own sources, the rest out of reach of every target: at most m correspondences
            gap = np.sqrt(((surface[:, None] - surface[None, :m]) ** 2).sum(2)).min(1) if m else np.full(len(surface), 1.0)
            rows = np.concatenate([np.arange(m), np.flatnonzero(gap > 2 * D)[:50 - m]])
        else:
            rows = rng.permutation(len(surface))[:50]
        assert len(rows) == 50
        srcs.append(surface[rows].astype(np.float32))
        tgts.append((surface[:m] @ T[:3, :3].T + T[:3, 3]).astype(np.float32).reshape(m, 3))
    kw = dict(max_iteration=MI, **PLANE)
    reads = REG.D2H_READS
    inside = REG.refine_batch(srcs, tgts, None, D, trace=True, normal_radius=R_NORMAL, **kw)
    assert REG.D2H_READS == reads + 1
    normals = REG.estimate_normals_batch(tgts, R_NORMAL, 30)
    for b, m in enumerate(RAGGED_M):
        assert inside.trace["normals"][b].shape == (m, 3) and torch.equal(inside.trace["normals"][b], normals[b]), m
    given = REG.refine_batch(srcs, tgts, None, D, trace=True, tgt_normals=normals, **kw)
    chunked = [REG.refine_batch(srcs, tgts, None, D, normal_radius=R_NORMAL, pairs_per_call=k, **kw) for k in (2, 4)]
    for b, m in enumerate(RAGGED_M):
        assert _five(inside, b) == _five(given, b) == _five(chunked[0], b) == _five(chunked[1], b), m
        possible = IR.evaluate(srcs[b], tgts[b], np.eye(4), D)[2]
        if m <= 3:
            assert possible < PR.MIN_COUNT, (m, possible)
            assert inside.iterations[b] == 0 and inside.matrices[b].tobytes() == np.eye(4).tobytes(), m
            assert inside.counts[b] == possible
        if m > 0:
            _check_steps(inside, b, srcs[b], tgts[b], normals[b].cpu().numpy(), np.eye(4), max_cond=None)
    assert inside.iterations[-1] >= 1
    assert torch.equal(torch.nan_to_num(inside.trace["sums27"], nan=-7.0), torch.nan_to_num(given.trace["sums27"], nan=-7.0))
