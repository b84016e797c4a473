"""GPU: the robust loss kernels of point-to-plane and colored ICP (csrc/icp.hip: pcrcg_icp_plane_robust_batch,
pcrcg_colored_icp_robust_batch, k_icp_evaluate<1, true> / <3, true>; csrc/robust_kernel.h; registration.RobustKernel,
robust_refine_batch, robust_colored_icp_batch and kernel= of refine / colored_icp) against the numpy restatement tests/robust_ref.py, in the manner of
tests/test_icp_plane_gpu.py: every T_k of the device's trace is fed into the restatement and one step is compared at a time.

  * L2Loss() is the plain entry (refine_batch, colored_icp_batch) bit for bit: results, statistics, every trace array;
  * each weighted kind, step by step: correspondences, counts and d2 sums as the plain tests pin them (the weights touch none
    of them), the 27 WEIGHTED sums within 1e-12 of the restated sums of the weighted terms' absolute values, T_k+1 within 1e-9
    of the restatement's solve where cond(A) <= 1e4 and within 1e-13 cond(A) beyond (tests/test_icp_plane_gpu.py's two bounds),
    the stop step;
  * batches, chunks and repeats give the same bits;
  * Tukey with every residual outside k: all weights 0, the system singular, the pair keeps its start;
  * L1 with every residual exactly 0: finite (the floor), and the pose stays;
  * the claim: with a quarter of the targets on a second sheet inside the gate, Huber, Cauchy and GM end within a third of
    the plain estimator's error -- asserted for the restatement first, so a failure says which side moved."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import colored_icp_ref as CR
from . import icp_plane_ref as PR
from . import icp_ref as IR
from . import robust_ref as RK
from .registration_cases import Recorder

pytestmark = pytest.mark.gpu

D, MI = 0.15, 10
PLANE = dict(estimation="point_to_plane")
# the five weighted kinds at the issue's scales: k = 0.005 (residuals are metres; the starts are a centimetre off), GM 1e-4
KERNELS = {"L1": (RK.L1, 1.0), "Huber": (RK.HUBER, 0.005), "Cauchy": (RK.CAUCHY, 0.005), "GM": (RK.GM, 1e-4), "Tukey": (RK.TUKEY, 0.005)}


def _kernel(name):
    kind, k = KERNELS[name]
    return REG.RobustKernel(kind, k)


def _host(trace, b):
    return {key: trace[key][b].cpu().numpy() for key in ("transforms", "counts", "sums", "corr", "sums27")}


def _five(res, b):
    """The five outputs of pair b, as bytes and numbers that compare bit for bit."""
    return (res.matrices[b].tobytes(), np.float64(res.fitness[b]).tobytes(), np.float64(res.inlier_rmse[b]).tobytes(),
            int(res.counts[b]), int(res.iterations[b]))


def _check_steps(res, b, src, tgt, T0, terms_at, min_count, d=D, mi=MI):
    """Pair b of a traced result against the restatement, one step at a time -> its host trace.  terms_at(T, corr) -> the
    restated weighted terms [count, 27]."""
    tr = _host(res.trace, b)
    n = len(src)
    iters = int(res.iterations[b])
    assert 0 <= iters <= mi
    assert np.array_equal(tr["transforms"][0], np.asarray(T0, np.float64))
    can_update = {}
    for k in range(iters + 1):
        Tk = tr["transforms"][k]
        corr, _, count, total = IR.evaluate(src, tgt, Tk, d)
        got = tr["corr"][k].astype(np.int64)
        assert (got == corr).all(), (k, np.flatnonzero(got != corr)[:5])
        assert tr["counts"][k] == count, k
        assert abs(tr["sums"][k] - total) <= 1e-12 * max(abs(total), 1e-300), k
        terms = terms_at(Tk, got)
        want, mag = RK.sums27(terms)
        assert np.isfinite(want).all(), k
        err = np.abs(tr["sums27"][k] - want)
        print("step", k, "count", count, "sums27 error / bound", float((err / np.maximum(1e-12 * mag, 1e-300)).max()) if count else 0.0)
        assert (err <= 1e-12 * mag).all(), (k, err, mag)
        delta, cond = RK.update(terms, min_count)
        can_update[k] = delta is not None
        if k < iters:
            assert delta is not None, k
            step = np.abs(tr["transforms"][k + 1] - delta @ Tk).max()
            bound = 1e-9 if cond <= 1e4 else 1e-13 * cond
            print("step", k, "cond", cond, "|T_k+1 - restated|", step, "bound", bound)
            assert step <= bound, (k, step, cond)
    assert IR.stop_iteration(tr["counts"], tr["sums"], n, lambda k: can_update[k], mi) == iters
    assert (tr["counts"][iters + 1:] == -1).all() and np.isnan(tr["transforms"][iters + 1:]).all()
    assert np.isnan(tr["sums27"][iters + 1:]).all()
    fit, rmse = IR.statistics(int(tr["counts"][iters]), float(tr["sums"][iters]), n)
    assert np.array_equal(res.matrices[b], tr["transforms"][iters])
    assert res.fitness[b] == fit and res.inlier_rmse[b] == rmse and res.counts[b] == tr["counts"][iters]
    return tr


# --- the data ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized():
    """icp_plane_ref.sized_pair of every size: (src, tgt, normals, start).  Do not write to it."""
    return {n: PR.sized_pair(i, n) for i, n in enumerate(PR.SIZES)}


@pytest.fixture(scope="module")
def resampled():
    """The corner cloud against an independent noisy sample of its image, with the sample's exact normals, from the identity."""
    src, tgt, T_gt = PR.corner_pair(n=1200, m=1500, noise=0.002)
    return src, tgt, PR.corner_normals(PR.corner(1000, 1500)) @ T_gt[:3, :3].T, np.eye(4)


def _plane_run(pairs, kernel, trace=False, **kw):
    """robust_refine_batch over (src, tgt, normals, start) tuples; kernel None: the plain entry itself, refine_batch."""
    kw.setdefault("max_iteration", MI)
    args = ([p[0] for p in pairs], [p[1] for p in pairs], np.stack([p[3] for p in pairs]), kw.pop("d", D))
    if kernel is None:
        return REG.refine_batch(*args, tgt_normals=[p[2] for p in pairs], trace=trace, **PLANE, **kw)
    return REG.robust_refine_batch(*args, kernel, tgt_normals=[p[2] for p in pairs], trace=trace, **kw)


def _colored_run(cases, kernel, trace=False, **kw):
    """colored_icp_batch over colored_icp_ref.case tuples (src, tgt, src RGB, tgt RGB, tgt normals, start, ...)."""
    kw.setdefault("max_iteration", MI)
    args = ([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], np.stack([c[5] for c in cases]), D)
    if kernel is None:
        return REG.colored_icp_batch(*args, tgt_normals=[c[4] for c in cases], trace=trace, **kw)
    return REG.robust_colored_icp_batch(*args, kernel, tgt_normals=[c[4] for c in cases], trace=trace, **kw)


def _same_traces(a, b, extra=()):
    for key in ("transforms", "counts", "sums", "sums27"):
        assert a.trace[key].cpu().numpy().tobytes() == b.trace[key].cpu().numpy().tobytes(), key
    for key in ("corr", "normals") + tuple(extra):
        assert len(a.trace[key]) == len(b.trace[key])
        for x, y in zip(a.trace[key], b.trace[key]):
            assert x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), key


# --- 1. L2 is the plain estimator -------------------------------------------------------------------------------------------
def test_l2_is_point_to_plane_bit_for_bit(cuda, sized):
    empty = (np.zeros((0, 3), np.float32), sized[7][1], sized[7][2], np.eye(4))
    pairs = [sized[n] for n in PR.SIZES] + [empty]
    plain = _plane_run(pairs, None, trace=True)
    l2 = _plane_run(pairs, REG.L2Loss(), trace=True)
    for b in range(len(pairs)):
        assert _five(l2, b) == _five(plain, b), b
    assert torch.equal(l2.transformations, plain.transformations)
    _same_traces(l2, plain)
    assert (plain.iterations[2:9] >= 1).all() and plain.iterations[9] == 0


def test_l2_is_colored_icp_bit_for_bit(cuda):
    cases = [CR.case("plane300")] + [CR.case(f"size{n}") for n in PR.SIZES]
    plain = _colored_run(cases, None, trace=True)
    l2 = _colored_run(cases, REG.L2Loss(), trace=True)
    for b in range(len(cases)):
        assert _five(l2, b) == _five(plain, b), b
    _same_traces(l2, plain, ("tgt_records", "src_intensities"))
    assert plain.iterations[0] >= 2 and (plain.iterations[3:] >= 2).all()


# --- 2. the weighted kinds, point-to-plane, step by step --------------------------------------------------------------------
@pytest.mark.parametrize("data", ["size7", "size513", "size1025", "resampled"])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_point_to_plane_steps_follow_the_restatement(cuda, sized, resampled, name, data):
    src, tgt, nrm, start = resampled if data == "resampled" else sized[int(data[4:])]
    kind, k = KERNELS[name]
    reads = REG.D2H_READS
    res = _plane_run([(src, tgt, nrm, start)], _kernel(name), trace=True)
    assert REG.D2H_READS == reads + 1
    assert res.trace["normals"][0].cpu().numpy().tobytes() == np.ascontiguousarray(nrm, np.float64).tobytes()
    _check_steps(res, 0, src, tgt, start, lambda T, corr: RK.plane_terms(src, tgt, nrm, T, corr, kind, k), PR.MIN_COUNT)
    run = RK.plane_icp(src, tgt, nrm, start, D, kind, k, max_iteration=MI)
    print(name, data, "updates", res.iterations[0], "restatement", run[4])
    assert res.iterations[0] == run[4] and res.counts[0] == run[3]
    if (name, data) == ("Tukey", "size7"):
        # three of the seven residuals lie beyond k at the start: four rows are left for six unknowns, the solve refuses
        assert res.iterations[0] == 0 and res.matrices[0].tobytes() == start.tobytes()
    else:
        assert res.iterations[0] >= 1
    # the kernel reaches the device: the plain estimator goes elsewhere from the first update on
    plain = _plane_run([(src, tgt, nrm, start)], None, trace=True)
    assert not np.array_equal(plain.trace["sums27"][0][0].cpu().numpy(), res.trace["sums27"][0][0].cpu().numpy())


# --- 3. the same for colored ICP ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["size7", "size513", "size1025", "plane300"])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_colored_steps_follow_the_restatement(cuda, name, data):
    case = CR.case(data)
    src, tgt, start = case[0], case[1], case[5]
    kind, k = KERNELS[name]
    reads = REG.D2H_READS
    res = _colored_run([case], _kernel(name), trace=True)
    assert REG.D2H_READS == reads + 1
    # the steps on the device's own records (tests/test_colored_icp_gpu.py pins those to the restated ones)
    rec, Is = res.trace["tgt_records"][0].cpu().numpy(), res.trace["src_intensities"][0].cpu().numpy()
    terms_at = lambda T, corr: RK.colored_terms(src, tgt, rec, Is, CR.LAMBDA, T, corr, kind, k)
    _check_steps(res, 0, src, tgt, start, terms_at, CR.MIN_COUNT)
    if (name, data) in (("Tukey", "size7"), ("L1", "plane300")):
        # Tukey leaves four of the seven geometric rows; on the exact plane every geometric residual is 0, L1 gives those rows
        # 1e12 against a colour row's ten or so, and the pivot rule (1e-12) refuses what is left of the in-plane unknowns
        assert res.iterations[0] == 0 and res.matrices[0].tobytes() == start.tobytes()
    else:
        assert res.iterations[0] >= 1
    plain = _colored_run([case], None, trace=True)
    assert plain.trace["tgt_records"][0].cpu().numpy().tobytes() == rec.tobytes()
    assert not np.array_equal(plain.trace["sums27"][0][0].cpu().numpy(), res.trace["sums27"][0][0].cpu().numpy())


# --- 4. batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Huber", "GM"])
def test_batches_chunks_and_repeats_give_the_same_bits(cuda, sized, resampled, name):
    pairs = [sized[1025], sized[7], resampled, sized[513], sized[5]]
    reads = REG.D2H_READS
    batch = _plane_run(pairs, _kernel(name))
    two = _plane_run(pairs, _kernel(name), pairs_per_call=2)
    assert REG.D2H_READS == reads + 2
    again = _plane_run(pairs, _kernel(name))
    for b, pair in enumerate(pairs):
        alone = _plane_run([pair], _kernel(name))
        assert _five(batch, b) == _five(alone, 0) == _five(two, b) == _five(again, b), b
    assert batch.iterations[4] == 0 and (batch.iterations[:4] >= 1).all()
    cases = [CR.case("size513"), CR.case("plane300"), CR.case("size1"), CR.case("size1025")]
    batch = _colored_run(cases, _kernel(name))
    two = _colored_run(cases, _kernel(name), pairs_per_call=2)
    again = _colored_run(cases, _kernel(name))
    for b, case in enumerate(cases):
        alone = _colored_run([case], _kernel(name))
        assert _five(batch, b) == _five(alone, 0) == _five(two, b) == _five(again, b), b
    assert batch.iterations[2] == 0 and (batch.iterations[[0, 1, 3]] >= 1).all()


# --- 5. Tukey, every residual outside ----------------------------------------------------------------------------------------
def test_tukey_with_every_residual_outside_keeps_the_start(cuda):
    src, tgt, nrm, _ = PR.plane_pair(tilted=True)
    start = np.eye(4)
    start[:3, 3] = 0.01 * nrm[0]
    d, k = 0.05, 0.005
    corr, _, count, total = IR.evaluate(src, tgt, start, d)
    assert count == len(src)
    _, res0 = RK.plain_plane_terms_of(IR.move(src, start).astype(np.float64), tgt[corr].astype(np.float64), nrm[corr])
    assert (np.abs(res0) >= k).all() and (RK.plane_terms(src, tgt, nrm, start, corr, RK.TUKEY, k) == 0.0).all()
    got = REG.robust_refine_batch([src], [tgt], start[None], d, REG.TukeyLoss(k), max_iteration=MI, trace=True, tgt_normals=[nrm])
    assert got.iterations[0] == 0 and got.matrices[0].tobytes() == start.tobytes()
    # fitness and rmse are those of Evaluate(start): of the device's own count and d2 sum, which equal the restated ones
    tr = _check_steps(got, 0, src, tgt, start, lambda T, c: RK.plane_terms(src, tgt, nrm, T, c, RK.TUKEY, k), PR.MIN_COUNT, d=d)
    assert got.fitness[0] == 1.0 and got.counts[0] == count and got.inlier_rmse[0] == IR.statistics(count, float(tr["sums"][0]), count)[1]
    assert abs(got.inlier_rmse[0] - 0.01) < 1e-6 and (tr["sums27"][0] == 0.0).all()
    # a pair the plain estimator does update (the corner, off by 0.02 along (1, 1, 1) / sqrt 3: 0.0115 from every face)
    src, tgt, T_gt = PR.corner_pair(n=1200)
    nrm = PR.corner_normals(PR.corner(0, 1200)) @ T_gt[:3, :3].T
    start = T_gt.copy()
    start[:3, 3] += T_gt[:3, :3] @ (0.02 * np.ones(3) / np.sqrt(3.0))
    corr, _, count, total = IR.evaluate(src, tgt, start, d)
    assert count >= 1000 and (RK.plane_terms(src, tgt, nrm, start, corr, RK.TUKEY, k) == 0.0).all()
    both = [REG.robust_refine_batch([src], [tgt], start[None], d, kern, max_iteration=MI, trace=True, tgt_normals=[nrm])
            for kern in (REG.TukeyLoss(k), None)]
    assert both[0].iterations[0] == 0 and both[0].matrices[0].tobytes() == start.tobytes()
    assert (both[0].trace["sums27"][0][0].cpu().numpy() == 0.0).all() and both[0].counts[0] == count
    assert both[1].iterations[0] >= 2 and PR.worst_displacement(src, both[1].matrices[0], T_gt) < 1e-6


# --- 6. L1 at exact zero residuals ----------------------------------------------------------------------------------------------
def test_l1_at_exact_zero_residuals_is_finite(cuda):
    """Targets that are the kernel's own fp32 images of the sources under the start: p = q bit for bit, every residual exactly 0,
    every weight 1 / kL1Floor.  open3d's 1 / |r| would make the system NaN; here b = 0, the step is the identity and the pose stays."""
    T_gt = PR.planted_pose()
    for i, n in ((2, 6), (6, 513), (8, 1025)):
        pts = PR.corner(200 + i, n)
        src = pts.astype(np.float32)
        order = np.random.RandomState(300 + i).permutation(n)
        tgt = IR.move(src, T_gt)[order]
        nrm = (PR.corner_normals(pts) @ T_gt[:3, :3].T)[order]
        corr = IR.evaluate(src, tgt, T_gt, D)[0]
        terms = RK.plane_terms(src, tgt, nrm, T_gt, corr, RK.L1, 1.0)
        assert (corr >= 0).all() and (terms[:, 21:] == 0.0).all() and np.isfinite(terms).all() and terms[:, :21].max() >= 1e11
        res = REG.robust_refine_batch([src], [tgt], T_gt[None], D, REG.L1Loss(), max_iteration=MI, trace=True, tgt_normals=[nrm])
        assert np.isfinite(res.matrices[0]).all() and np.isfinite(res.trace["sums27"][0][0].cpu().numpy()).all()
        assert res.fitness[0] == 1.0 and res.inlier_rmse[0] == 0.0 and res.counts[0] == n
        assert PR.worst_displacement(src, res.matrices[0], T_gt) <= 1e-12, n
        _check_steps(res, 0, src, tgt, T_gt, lambda T, c: RK.plane_terms(src, tgt, nrm, T, c, RK.L1, 1.0), PR.MIN_COUNT)


# --- 7. the outlier scene ---------------------------------------------------------------------------------------------------------
CLAIM = {"plain": None, "Huber": (RK.HUBER, 0.005), "Cauchy": (RK.CAUCHY, 0.005), "GM": (RK.GM, 1e-4)}
TUKEY_SCENE, TUKEY_K = (1, 600), 0.015


@pytest.fixture(scope="module")
def outlier_runs(cuda):
    """name -> the device's result on all six scenes in one batch (30 iterations, d = 0.06); Tukey on its one scene."""
    scenes = [RK.outlier_scene(*s) for s in RK.OUTLIER_SCENES]
    out = {name: _plane_run(scenes, None if spec is None else REG.RobustKernel(*spec), max_iteration=RK.OUTLIER_MI, d=RK.OUTLIER_D)
           for name, spec in CLAIM.items()}
    out["Tukey"] = _plane_run([RK.outlier_scene(*TUKEY_SCENE)], REG.TukeyLoss(TUKEY_K), max_iteration=RK.OUTLIER_MI, d=RK.OUTLIER_D)
    return out


@pytest.mark.parametrize("scene", RK.OUTLIER_SCENES)
def test_the_robust_kinds_end_within_a_third_of_the_plain_error(cuda, outlier_runs, scene):
    src, tgt, nrm, start, T_gt = RK.outlier_scene(*scene)
    b = RK.OUTLIER_SCENES.index(scene)
    ref, dev = {}, {}
    for name, spec in CLAIM.items():
        kind, k = (RK.L2, 1.0) if spec is None else spec
        ref[name] = PR.worst_displacement(src, RK.plane_icp(src, tgt, nrm, start, RK.OUTLIER_D, kind, k, max_iteration=RK.OUTLIER_MI)[0], T_gt)
        dev[name] = PR.worst_displacement(src, outlier_runs[name].matrices[b], T_gt)
    print(scene, "restatement (mm)", {n: round(1e3 * v, 3) for n, v in ref.items()}, "device (mm)", {n: round(1e3 * v, 3) for n, v in dev.items()})
    for name in ("Huber", "Cauchy", "GM"):
        assert ref[name] < ref["plain"] / 3, ("restatement", name, ref)
    for name in ("Huber", "Cauchy", "GM"):
        assert dev[name] < dev["plain"] / 3, ("device", name, dev)
    if scene == TUKEY_SCENE:
        # Tukey on this scene alone: it is not convex, and on (seed 0, n 1200) the restatement itself locks onto the displaced
        # sheet -- its known behaviour from a start between two sheets, not a defect; that scene is left out for it
        r = PR.worst_displacement(src, RK.plane_icp(src, tgt, nrm, start, RK.OUTLIER_D, RK.TUKEY, TUKEY_K, max_iteration=RK.OUTLIER_MI)[0], T_gt)
        g = PR.worst_displacement(src, outlier_runs["Tukey"].matrices[0], T_gt)
        print(scene, "Tukey: restatement (mm)", round(1e3 * r, 3), "device (mm)", round(1e3 * g, 3))
        assert r < ref["plain"] / 3 and g < dev["plain"] / 3


# --- 8. plumbing ------------------------------------------------------------------------------------------------------------------
def test_which_entry_a_call_makes_and_what_it_reads(cuda, sized):
    pair = sized[513]
    for kernel, entry in ((None, "pcrcg_icp_batch_ex"), (REG.HuberLoss(0.0075), "pcrcg_icp_plane_robust_batch")):
        reads = REG.D2H_READS
        with Recorder() as rec:
            _plane_run([pair, sized[7]], kernel, pairs_per_call=1)
        assert REG.D2H_READS == reads + 1
        icp = [c for c in rec.log if "icp" in c[0] and not c[0].endswith("ws_bytes")]
        assert [c[0] for c in icp] == [entry, entry]
        if kernel is None:
            assert [c[14:16] for c in icp] == [[1, "ptr"], [1, "ptr"]]                   # estimation, tgt_normals
        else:
            assert [c[14:17] for c in icp] == [["ptr", 2, 0.0075], ["ptr", 2, 0.0075]]    # tgt_normals, kernel, kernel_k
    # kernel=None through the robust entries is the plain call: the same entry, the same arguments
    logs = []
    for call in (lambda: _plane_run([pair], None), lambda: REG.robust_refine_batch([pair[0]], [pair[1]], pair[3][None], D, None,
                                                                                   max_iteration=MI, tgt_normals=[pair[2]])):
        with Recorder() as rec:
            call()
        logs.append([c for c in rec.log if "icp" in c[0]])
    assert logs[0] == logs[1] and [c[0] for c in logs[0]] == ["pcrcg_icp_batch_ex_ws_bytes", "pcrcg_icp_batch_ex"]
    case = CR.case("size513")
    for kernel, entry in ((None, "pcrcg_colored_icp_batch"), (REG.HuberLoss(0.0075), "pcrcg_colored_icp_robust_batch")):
        reads = REG.D2H_READS
        with Recorder() as rec:
            _colored_run([case], kernel)
        assert REG.D2H_READS == reads + 1
        icp = [c for c in rec.log if "icp" in c[0] and not c[0].endswith("ws_bytes")]
        assert [c[0] for c in icp] == [entry]
        assert icp[0][14:17] == [CR.LAMBDA, "ptr", "ptr"]
        if kernel is not None:
            assert icp[0][17:19] == [2, 0.0075]


def test_the_single_pair_wrappers_equal_the_batch_of_one(cuda, sized):
    src, tgt, nrm, start = sized[1025]
    kern = REG.CauchyLoss(0.005)
    one = _plane_run([sized[1025]], kern)
    single = REG.refine(src, tgt, start, D, max_iteration=MI, tgt_normals=nrm, kernel=kern, **PLANE)
    assert (single.matrix.tobytes(), single.iterations, single.fitness) == (one.matrices[0].tobytes(), one.iterations[0], one.fitness[0])
    assert single.iterations >= 1
    c = CR.case("size1025")
    one = _colored_run([c], kern)
    single = REG.colored_icp(c[0], c[1], c[2], c[3], c[5], D, tgt_normals=c[4], max_iteration=MI, kernel=kern)
    assert (single.matrix.tobytes(), single.iterations, single.fitness) == (one.matrices[0].tobytes(), one.iterations[0], one.fitness[0])
    assert single.iterations >= 1
