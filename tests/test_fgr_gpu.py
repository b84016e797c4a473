"""GPU: registration.mutual_match_batch and fast_global_registration_batch (csrc/register.hip, csrc/fgr.hip) against the numpy
float64 restatement tests/fgr_ref.py, stage by stage through the trace.

Tolerances.  The mutual list, the accepted trials, E, the counts and mu's schedule are exact (tests/test_fgr_cpu.py asserts that
no edge test of these inputs is decided by less than a relative 1e-9).  Per iteration, as tests/test_icp_plane_gpu.py: each of
the 27 sums within 1e-12 of the sum of its terms' absolute values (a few hundred float64 additions in another order), the next
T within 1e-9 of the restatement's step from the device's own T and mu, cond(A) <= 1e4.  End to end: the final pose within
iteration_number x 1e-9 of the restatement's own run."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import fgr_ref as FR
from . import fpfh_ref as FPR
from . import registration_cases as RC
from .ransac_ref import pose_error

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12
STEP_TOL = 1e-9
COND_CAP = 1e4


def _np(t):
    return t.cpu().numpy()


# --- 1. mutual match -----------------------------------------------------------------------------------------------------
def _check_lists(fs, ft, corr, k):
    """corr / k of mutual_match_batch(fs, ft) against the restatement fed the device's own two nearest-neighbour lists."""
    ns, ms = [len(x) for x in fs], [len(x) for x in ft]
    corr, k = _np(corr), _np(k)
    assert corr.shape == (sum(ns), 2) and corr.dtype == np.int32 and k.shape == (len(ns),)
    live = [b for b in range(len(ns)) if ns[b] and ms[b]]
    fwd = _np(REG.feature_match_batch([fs[b] for b in live], [ft[b] for b in live])[0])[:, 1]
    bwd = _np(REG.feature_match_batch([ft[b] for b in live], [fs[b] for b in live])[0])[:, 1]
    fwd = dict(zip(live, np.split(fwd, np.cumsum([ns[b] for b in live])[:-1])))
    bwd = dict(zip(live, np.split(bwd, np.cumsum([ms[b] for b in live])[:-1])))
    at = 0
    for b in range(len(ns)):
        rows = corr[at:at + ns[b]]
        at += ns[b]
        if b in live:
            want, kw = FR.mutual_list(fwd[b], bwd[b], ns[b], ms[b])
            assert kw >= 1          # the closest pair of a non-empty pair is always mutual
        else:
            want, kw = np.full((ns[b], 2), -1, np.int32), 0
        assert k[b] == kw and np.array_equal(rows, want), b


@pytest.mark.parametrize("c", [32, 33])
def test_mutual_match_equals_both_nearest_neighbour_lists(c):
    """The five ragged pairs of tests/registration_cases.py at width 32 (matrix cores) and 33 (FPFH's, the generic kernel): the
    list is the restatement's of feature_match_batch's rows in both directions, equals the float64 rule (random normal
    descriptors decide every neighbour far above fp32 rounding), and each pair alone equals its rows in the batch."""
    d = RC.inputs()
    fs, ft = d[f"fs{c}"], d[f"ft{c}"]
    corr, k = REG.mutual_match_batch(fs, ft)
    _check_lists(fs, ft, corr, k)
    corr, k = _np(corr), _np(k)
    at = 0
    for b, (a, bb) in enumerate(zip(fs, ft)):
        want, kw = FR.mutual_match(a, bb)
        assert k[b] == kw and np.array_equal(corr[at:at + len(a)], want)
        alone = REG.mutual_match_batch([a], [bb])
        assert np.array_equal(_np(alone[0]), want) and int(_np(alone[1])[0]) == kw
        at += len(a)


@pytest.mark.parametrize("c", [2, 32])
def test_mutual_match_ties_take_the_lowest_index(c):
    """Small integers, exact in fp32: source rows 0 and 1 are equal, target rows 0, 1 and 2, 3 are equal pairs.  nn_s = (0, 0, 2),
    nn_t = (0, 0, 2, 2): rows 0 and 2 are mutual, row 1 loses target 0 to row 0."""
    a = np.zeros((3, c), np.float32)
    b = np.zeros((4, c), np.float32)
    a[0, 0] = a[1, 0] = a[2, 1] = 2.0
    b[0, 0] = b[1, 0] = b[2, 1] = b[3, 1] = 2.0
    corr, k = REG.mutual_match_batch([a], [b])
    assert int(_np(k)[0]) == 2 and _np(corr).tolist() == [[0, 0], [2, 2], [-1, -1]]
    assert FR.mutual_match(a, b)[0].tolist() == [[0, 0], [2, 2], [-1, -1]]


def test_mutual_match_pairs_with_an_empty_side():
    """k = 0 needs an empty side: with both sides non-empty the closest pair (lowest indices among equals) is mutual, so k >= 1.
    A pair with no source rows, one with no target rows (its rows all (-1, -1)) and a full pair between them."""
    rng = np.random.RandomState(5)
    fs = [np.zeros((0, 33), np.float32), rng.randn(70, 33).astype(np.float32), rng.randn(9, 33).astype(np.float32)]
    ft = [rng.randn(12, 33).astype(np.float32), rng.randn(300, 33).astype(np.float32), np.zeros((0, 33), np.float32)]
    corr, k = REG.mutual_match_batch(fs, ft)
    _check_lists(fs, ft, corr, k)
    assert _np(k)[0] == 0 and _np(k)[2] == 0 and (_np(corr)[70:] == -1).all()
    corr, k = REG.mutual_match_batch(fs[2:], ft[2:])           # no target row in the whole call
    assert _np(k).tolist() == [0] and (_np(corr) == -1).all()


# --- 2 .. 4: the registration against the restatement ------------------------------------------------------------------------
def _run(cases, seeds=0, trace=True, **extra):
    kw = dict(cases[0]["kw"], **extra)
    assert all(c["kw"] == cases[0]["kw"] for c in cases)
    return REG.fast_global_registration_batch([c["src"] for c in cases], [c["tgt"] for c in cases],
                                              correspondences=[c["corr"] for c in cases], seeds=seeds, trace=trace, **kw)


def _stats(res, b=0):
    return [int(res.n_correspondences[b]), int(res.tuples[b]), int(res.trials[b]), int(res.updates[b]), float(res.mu[b]),
            float(res.inlier_share[b])]


def _check_tuples(res, ref, b=0):
    """The accepted trials, E and the three counts of pair b, exactly."""
    tr = res.trace
    trials, entries = _np(tr["trials"][b]), _np(tr["entries"][b])
    n_acc, nE = ref["tuples"]["accepted"], len(ref["tuples"]["E"])
    assert np.array_equal(trials[:n_acc], ref["tuples"]["trials"]) and (trials[n_acc:] == -1).all()
    assert np.array_equal(entries[:nE], ref["tuples"]["E"]) and (entries[nE:] == -1).all()
    assert _stats(res, b)[:3] == ref["stats"][:3]


@pytest.mark.parametrize("name", sorted(FR.TUPLE_CASES))
def test_tuple_stage(name):
    c = FR.TUPLE_CASES[name]()
    ref = FR.run_case(c)
    res = _run([c])
    _check_tuples(res, ref)
    assert _stats(res)[3] == ref["stats"][3]
    if len(ref["tuples"]["E"]) < FR.MIN_ENTRIES:
        assert np.array_equal(res.matrices[0], np.eye(4)) and _stats(res)[3:] == [0, 0.0, 0.0]
        assert torch.isnan(res.trace["frame"][0]).all() and torch.isnan(res.trace["mu"][0]).all()
    else:
        _check_steps(res, ref, c)


def _check_steps(res, ref, c, b=0):
    """Every traced iteration of pair b recomputed by the restatement from the device's own frame, T_it and mu_it."""
    tr, kw = res.trace, c["kw"]
    E = ref["tuples"]["E"]
    fr = _np(tr["frame"][b])
    cs, ct, D2 = fr[:3], fr[3:6], fr[6]
    p, q = c["src"].astype(np.float64)[E[:, 0]], c["tgt"].astype(np.float64)[E[:, 1]]
    ref_cs, ref_ct, _ = FR.frame(p, q)
    scale = max(np.abs(p).max(), np.abs(q).max())
    assert np.abs(cs - ref_cs).max() <= SUM_TOL * scale and np.abs(ct - ref_ct).max() <= SUM_TOL * scale
    pt, qt = p - cs, q - ct
    n2 = lambda v: (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    assert D2 == max(n2(pt).max(), n2(qt).max())
    Ts, mus, sums = _np(tr["transforms"][b]), _np(tr["mu"][b]), _np(tr["sums27"][b])
    ran = int(np.isfinite(mus).sum())
    assert np.isfinite(mus[:ran]).all() and ran >= 1 and mus[0] == D2 and np.array_equal(Ts[0], np.eye(4))
    delta, div, dec = kw["maximum_correspondence_distance"], kw.get("division_factor", 1.4), kw.get("decrease_mu", True)
    updates, T_next = 0, None
    for it in range(ran):
        st = FR.step(pt, qt, Ts[it], mus[it])
        assert st["cond"] <= COND_CAP or st["T_next"] is None
        assert (np.abs(sums[it] - st["sums"]) <= SUM_TOL * st["abs_sums"]).all(), it
        if st["T_next"] is None:
            assert it == ran - 1
            T_next = Ts[it]
            break
        updates += 1
        T_next = st["T_next"]
        if it + 1 < ran:
            assert np.abs(Ts[it + 1] - T_next).max() <= STEP_TOL, it
            assert mus[it + 1] == FR.next_mu(mus[it], it, delta, div, dec), it
    assert int(res.updates[b]) == updates
    assert np.abs(res.matrices[b] - FR.output(T_next, cs, ct)).max() <= STEP_TOL
    if updates == ran:
        assert float(res.mu[b]) == FR.next_mu(mus[ran - 1], ran - 1, delta, div, dec)
    return ran, mus


@pytest.mark.parametrize("name", sorted(FR.OPTIMISER_CASES))
def test_optimiser_step_by_step(name):
    c = FR.OPTIMISER_CASES[name]()
    ref = FR.run_case(c)
    res = _run([c])
    _check_tuples(res, ref)
    if name == "one_row":           # every entry the same row: D2 = 0, the frame rule gives the identity before any iteration
        assert np.array_equal(res.matrices[0], np.eye(4)) and _stats(res)[3:] == [0, 0.0, 0.0]
        assert float(_np(res.trace["frame"][0])[6]) == 0.0
        return
    ran, mus = _check_steps(res, ref, c)
    d2 = c["kw"]["maximum_correspondence_distance"] ** 2
    if name == "two_rows":          # collinear entries: the first solve fails, T stays the identity of the centred frame
        assert ran == 1 and _stats(res)[3] == 0 and np.array_equal(res.matrices[0][:3, :3], np.eye(3))
    elif name == "fixed_mu":
        assert ran == 64 and (mus == mus[0]).all() and float(res.mu[0]) == mus[0]
    elif name == "E4200_workspace":
        assert ran == 64 and len(ref["tuples"]["E"]) == 4200
    else:                           # mu comes down to delta^2 and stops there, well before the last iteration
        assert ran == 64 and mus[0] > d2 and float(res.mu[0]) <= d2 and mus[-1] == mus[-8] == float(res.mu[0])
    assert abs(_stats(res)[5] - ref["stats"][5]) <= 1.0 / len(ref["tuples"]["E"]) + 1e-12


def test_end_to_end_planted_poses():
    """The four scenarios of the CPU test: the device's final pose within iteration_number x 1e-9 of the restatement's own run
    (64 steps of at most 1e-9 each, and the steps do not expand), and the planted pose recovered within the CPU test's bars."""
    names = sorted(FR.SCENARIOS)
    for mtc in sorted({FR.SCENARIOS[n][3] for n in names}):
        group = [n for n in names if FR.SCENARIOS[n][3] == mtc]
        cases = []
        for n in group:
            src, tgt, corr, T, _ = FR.planted(n)
            cases.append({"src": src, "tgt": tgt, "corr": corr, "T": T,
                          "kw": {"maximum_correspondence_distance": FR.DELTA, "maximum_tuple_count": mtc}})
        res = _run(cases)
        for b, (n, c) in enumerate(zip(group, cases)):
            ref = FR.run_case(c)
            _check_tuples(res, ref, b)
            diff = np.abs(res.matrices[b] - ref["T"]).max()
            rot, trans = pose_error(res.matrices[b], c["T"])
            print(n, "device - restatement", diff, "rotation error", rot, "deg, translation error", trans, "m")
            assert _stats(res, b)[3] == 64 and abs(float(res.mu[b]) - ref["stats"][4]) <= 1e-12 * ref["stats"][4]
            assert diff <= 64 * STEP_TOL
            assert rot < 0.1 and trans < 0.005
            _check_steps(res, ref, c, b)


# --- 5. independence and determinism ---------------------------------------------------------------------------------------
def _bits(res, b):
    return res.matrices[b].tobytes() + np.asarray(_stats(res, b)[4:]).tobytes() + bytes(str(_stats(res, b)[:4]), "ascii")


def test_pairs_are_independent_and_runs_are_deterministic(monkeypatch):
    """B = 5 ragged pairs, pair 2 with an empty list (k = 0: the identity), pair 3 with a seed of 2^24 (the host check is lifted
    for it: the device answers with NaN in all 22 outputs).  Every pair equals its own call, the batch two pairs per call, the
    batch reversed, a second run, and every form of input; each call reads the device once, and refine_batch takes the result
    as its start with no read but its own."""
    monkeypatch.setattr(REG.ragged, "seed_list", lambda seeds, n, *a, **k: [int(s) for s in seeds])
    cases, seeds = FR.ragged_batch()
    before = REG.D2H_READS
    res = _run(cases, seeds, trace=False)
    assert REG.D2H_READS == before + 1
    assert np.isnan(res.matrices[3]).all() and np.isnan(res.mu[3]) and np.isnan(res.inlier_share[3])
    assert [int(x[3]) for x in (res.n_correspondences, res.tuples, res.trials, res.updates)] == [-1] * 4
    assert np.array_equal(res.matrices[2], np.eye(4)) and _stats(res, 2) == [0, 0, 0, 0, 0.0, 0.0]
    for b in (0, 1, 4):
        assert _stats(res, b)[3] == 64 and pose_error(res.matrices[b], cases[b]["T"])[0] < 0.1
    want = [_bits(res, b) for b in range(5)]
    for b in range(5):
        assert _bits(_run([cases[b]], [seeds[b]], trace=False), 0) == want[b], b
    before = REG.D2H_READS
    chunked = _run(cases, seeds, trace=False, pairs_per_call=2)
    assert REG.D2H_READS == before + 1
    rev = _run(cases[::-1], seeds[::-1], trace=False)
    again = _run(cases, seeds, trace=False)
    assert [_bits(chunked, b) for b in range(5)] == want and [_bits(again, b) for b in range(5)] == want
    assert [_bits(rev, 4 - b) for b in range(5)] == want
    dev = torch.device("cuda", torch.cuda.current_device())
    for form in RC.FORMS:
        got = REG.fast_global_registration_batch(
            RC.place([c["src"] for c in cases], form, dev), RC.place([c["tgt"] for c in cases], form, dev),
            correspondences=RC.place([c["corr"] for c in cases], form, dev), seeds=seeds, **cases[0]["kw"])
        assert [_bits(got, b) for b in range(5)] == want, form
    live = [0, 1, 2, 4]
    start = _run([cases[b] for b in live], [seeds[b] for b in live], trace=False)
    before = REG.D2H_READS
    fine = REG.refine_batch([cases[b]["src"] for b in live], [cases[b]["tgt"] for b in live], start, 0.05, max_iteration=5)
    assert REG.D2H_READS == before + 1
    same = REG.refine_batch([cases[b]["src"] for b in live], [cases[b]["tgt"] for b in live], start.matrices, 0.05, max_iteration=5)
    assert fine.matrices.tobytes() == same.matrices.tobytes()


def test_single_pair_wrapper_and_descriptor_path():
    """fast_global_registration is the batch of one; descriptors go through mutual_match_batch in the same call (one read)."""
    d = RC.inputs()
    src, tgt, fs, ft = d["src"][2], d["tgt"][2], d["fs33"][2], d["ft33"][2]
    before = REG.D2H_READS
    one = REG.fast_global_registration(src, tgt, fs, ft, maximum_correspondence_distance=0.05, seed=7, trace=True)
    assert REG.D2H_READS == before + 1
    corr, k = REG.mutual_match_batch([fs], [ft])
    assert torch.equal(one.trace["corr"][0], corr) and torch.equal(one.trace["k"][0], k)
    kk = int(_np(k)[0])
    by_list = REG.fast_global_registration_batch([src], [tgt], correspondences=[_np(corr)[:kk]], seeds=[7],
                                                 maximum_correspondence_distance=0.05)
    assert one.matrix.tobytes() == by_list.matrices[0].tobytes() and one.n_correspondences == kk
    ref = FR.fgr(src, tgt, _np(corr), kk, 0.05, seed=7)
    assert [one.n_correspondences, one.tuples, one.trials] == ref["stats"][:3]


# --- 6. from FPFH alone ----------------------------------------------------------------------------------------------------
def test_registration_from_fpfh_alone():
    """The height field of tests/test_fpfh_gpu.py's registration case and its copy under a signed axis permutation and a dyadic
    translation: compute_fpfh_feature_batch -> fast_global_registration_batch lands every source point within delta of its
    image.  First the same on the restatement fed the same features, so the condition is one the definition itself meets."""
    src, ns = FPR.height_field()
    R = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    t = np.array([4.0, -8.0, 2.0])
    perm = np.random.RandomState(9).permutation(len(src))
    moved = (src.astype(np.float64) @ R.T + t).astype(np.float32)
    tgt, nt = moved[perm], (ns @ R.T)[perm]
    delta = 0.05
    fs, ft = REG.compute_fpfh_feature_batch([src, tgt], 0.25, 128, normals=[ns, nt])

    def worst(T):
        return np.linalg.norm(src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - moved.astype(np.float64), axis=1).max()

    corr, k = FR.mutual_match(_np(fs), _np(ft))
    ref = FR.fgr(src, tgt, corr, k, delta, seed=3)
    assert ref["tuples"]["margin"] >= 1e-9
    print("restatement: k", k, "stats", ref["stats"], "worst point", worst(ref["T"]))
    assert worst(ref["T"]) < delta
    res = REG.fast_global_registration_batch([src], [tgt], [fs], [ft], maximum_correspondence_distance=delta, seeds=3, trace=True)
    print("device: stats", _stats(res), "worst point", worst(res.matrices[0]))
    assert worst(res.matrices[0]) < delta
    # the exact comparisons run on the device's own list (fp32 scores; the float64 rule above may differ on a near-tie)
    dcorr, dk = _np(res.trace["corr"][0]), int(_np(res.trace["k"][0])[0])
    print("lists equal:", dk == k and np.array_equal(dcorr, corr))
    ref = FR.fgr(src, tgt, dcorr, dk, delta, seed=3)
    assert ref["tuples"]["margin"] >= 1e-9
    _check_tuples(res, ref)
    assert np.abs(res.matrices[0] - ref["T"]).max() <= 64 * STEP_TOL
